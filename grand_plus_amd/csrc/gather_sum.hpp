// gather_sum.hpp -- the gather half of sort-then-gather, stated once for scatter_det.hip (§7i) and
// mag_det.hip (§7o): every destination row that occurs in a list of keys sorted by a stable sort is summed sequentially
// in that order, from 0.0f, by one wave, and written once with plain stores.  What one sorted position contributes is
// the unit's own Op (load / add, described in scatter_det.hip).  Everything has internal linkage, as in gp_common.hpp.
#pragma once

#include "gp_common.hpp"

#include <algorithm>

namespace {

constexpr int kGather = 64;           // gather_sum_kernel: one wave per workgroup, so that few windows still spread over the CUs
constexpr int kCols = 4;              // 64-column slabs of the destination row per pass of a segment

__device__ __forceinline__ int run_length(u64 same)                 // how many of the lowest bits are set
{
    return ~same ? __builtin_ctzll(~same) : 64;
}

// dst[dest, 0:W] = the sequential sum, from 0.0f, of the entries of dest's segment of the sorted list, for every key
// dest in [0, n_dest) that occurs.  One wave per workgroup; windows grid-stride.
template <class Op>
__global__ void __launch_bounds__(kGather)
gather_sum_kernel(Op op, const long long* __restrict__ order, const long long* __restrict__ keys, long long n_sorted,
                  long long n_dest, int W, float* __restrict__ dst)
{
    const int lane = threadIdx.x;
    const long long n_win = (n_sorted + 63) >> 6;
    for (long long win = blockIdx.x; win < n_win; win += gridDim.x) {          // wave-uniform
        const long long base = win << 6, i = base + lane;
        const long long key = i < n_sorted ? keys[i] : n_dest;
        const bool valid = key >= 0 && key < n_dest;
        u64 heads = __ballot(valid && (i == 0 || keys[i - 1] != key));
        if (!heads) continue;
        const typename Op::Entry mine = op.load(order, i, valid, key);
        while (heads) {
            const int l = __builtin_ctzll(heads);
            heads &= heads - 1;
            const long long dest = __shfl(key, l);
            const int n0 = run_length(__ballot(key == dest) >> l);            // the segment's entries inside the window
            float* out = dst + (size_t)dest * W;
            for (int f0 = 0; f0 < W; f0 += 64 * kCols) {
                float acc[kCols];
#pragma unroll
                for (int c = 0; c < kCols; ++c) acc[c] = 0.0f;
                for (int u = 0; u < n0; ++u) op.add(mine, l + u, f0 + lane, acc);
                if (l + n0 == 64) {                                               // it may run on past the window
                    for (long long pos = base + 64; pos < n_sorted; pos += 64) {
                        const long long q = pos + lane;
                        const int n = run_length(__ballot(q < n_sorted && keys[q] == dest));
                        if (n == 0) break;
                        const typename Op::Entry next = op.load(order, q, lane < n, dest);
                        for (int u = 0; u < n; ++u) op.add(next, u, f0 + lane, acc);
                        if (n < 64) break;
                    }
                }
#pragma unroll
                for (int c = 0; c < kCols; ++c)
                    if (f0 + 64 * c + lane < W) out[f0 + 64 * c + lane] = acc[c];
            }
        }
    }
}

int gather_grid(int64_t n_sorted) { return (int)std::min<int64_t>(65535, (n_sorted + 63) / 64); }

}  // namespace
