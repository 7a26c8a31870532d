// gather_chunk.hpp -- the chunked gather: gather_sum.hpp's sort-then-gather with every segment cut into
// chunks of C sorted positions, so that the serial chain of a hub destination is C adds plus ceil(n / C) adds instead of
// n.  Two launches, for the same Ops as gather_sum_kernel:
//   gather_chunk_kernel<Op>   a wave per window of 64 sorted positions.  Its heads are gather_sum_kernel's heads plus every
//                             position that starts a later chunk of its segment; a head's wave walks at most C positions.
//                             Chunk 0 of a segment of at most C positions goes to dst, as gather_sum_kernel writes it; every
//                             chunk of a longer segment goes to a scratch row;
//   gather_fold_kernel        the head of every longer segment sums its scratch rows in chunk order and stores dst.
// The order contract is stated in gather_chunk_abi.hpp, the chunk / slot / size arithmetic is gather_chunk_layout.hpp's
// (HIP-free, held on the CPU by tests/native/gather_chunk_check.cpp).  Plain stores only; nothing allocates, reads back or
// synchronises.  Everything has internal linkage, as in gp_common.hpp.
#pragma once

#include "gather_sum.hpp"
#include "gather_chunk_layout.hpp"

namespace {

constexpr int kFoldLoads = 8;         // gather_fold_kernel: scratch rows in flight per lane and column slab

template <class Op>
__global__ void __launch_bounds__(kGather)
gather_chunk_kernel(Op op, const long long* __restrict__ order, const long long* __restrict__ keys, long long n_sorted,
                    long long n_dest, int W, int C, float* __restrict__ dst, float* __restrict__ scratch)
{
    namespace gc = gp_gather_chunk;
    const int lane = threadIdx.x;
    const long long n_win = (n_sorted + 63) >> 6;
    for (long long win = blockIdx.x; win < n_win; win += gridDim.x) {          // wave-uniform
        const long long base = win << 6, i = base + lane;
        const long long key = i < n_sorted ? keys[i] : n_dest;
        const bool valid = key >= 0 && key < n_dest;
        const bool first = valid && (i == 0 || keys[i - 1] != key);              // gather_sum_kernel's head
        const u64 firsts = __ballot(first);
        // Only the run that enters the window from before it starts outside: one lane finds where.
        long long entered = base;
        if (__ballot(valid && !first) & 1) {                                     // wave-uniform: lane 0 goes on a run
            if (lane == 0) entered = gc::seg_start_of(keys, base, key);
            entered = __shfl(entered, 0);
        }
        const u64 below = firsts & (~0ull >> (63 - lane));                       // the firsts at or below this lane
        const long long seg_start = below ? base + (63 - __builtin_clzll(below)) : entered;
        u64 heads = __ballot(valid && gc::starts_chunk(i, seg_start, C));
        if (!heads) continue;
        const u64 longs = __ballot(first && gc::is_long(keys, n_sorted, i, key, C));
        const typename Op::Entry mine = op.load(order, i, valid, key);
        while (heads) {
            const int l = __builtin_ctzll(heads);
            heads &= heads - 1;
            const long long dest = __shfl(key, l), q = base + l;
            const long long p = gc::chunk_of(q, __shfl(seg_start, l), C);
            const int n0 = run_length(__ballot(key == dest) >> l);            // the chunk's entries inside the window: C >= 64
            float* out = p == 0 && !((longs >> l) & 1) ? dst + (size_t)dest * W : scratch + (size_t)gc::slot_of(q, p, C) * W;
            for (int f0 = 0; f0 < W; f0 += 64 * kCols) {
                float acc[kCols];
#pragma unroll
                for (int c = 0; c < kCols; ++c) acc[c] = 0.0f;
                for (int u = 0; u < n0; ++u) op.add(mine, l + u, f0 + lane, acc);
                int left = C - n0;                                                // positions the chunk may still take
                if (l + n0 == 64 && left > 0) {                                   // it may run on past the window
                    for (long long pos = base + 64; pos < n_sorted; pos += 64) {
                        const long long qq = pos + lane;
                        const int n = min(run_length(__ballot(qq < n_sorted && keys[qq] == dest)), left);
                        if (n == 0) break;
                        const typename Op::Entry next = op.load(order, qq, lane < n, dest);
                        for (int u = 0; u < n; ++u) op.add(next, u, f0 + lane, acc);
                        left -= n;
                        if (n < 64 || left == 0) break;
                    }
                }
#pragma unroll
                for (int c = 0; c < kCols; ++c)
                    if (f0 + 64 * c + lane < W) out[f0 + 64 * c + lane] = acc[c];
            }
        }
    }
}

// dst[dest, 0:W] = the sequential sum, from 0.0f, of the scratch rows of dest's chunks in chunk order, for every dest whose
// segment has more than C positions.  The rows lie at independent addresses: kFoldLoads of them are loaded before the
// first is added; the adds stay in order.
__global__ void __launch_bounds__(kGather)
gather_fold_kernel(const long long* __restrict__ keys, long long n_sorted, long long n_dest, int W, int C,
                   const float* __restrict__ scratch, float* __restrict__ dst)
{
    namespace gc = gp_gather_chunk;
    const int lane = threadIdx.x;
    const long long n_win = (n_sorted + 63) >> 6;
    for (long long win = blockIdx.x; win < n_win; win += gridDim.x) {          // wave-uniform
        const long long base = win << 6, i = base + lane;
        const long long key = i < n_sorted ? keys[i] : n_dest;
        const bool valid = key >= 0 && key < n_dest;
        const bool first = valid && (i == 0 || keys[i - 1] != key);
        u64 heads = __ballot(first && gc::is_long(keys, n_sorted, i, key, C));
        while (heads) {
            const int l = __builtin_ctzll(heads);
            heads &= heads - 1;
            const long long dest = __shfl(key, l), q0 = base + l;
            float* out = dst + (size_t)dest * W;
            for (int f0 = 0; f0 < W; f0 += 64 * kCols) {
                float acc[kCols];
#pragma unroll
                for (int c = 0; c < kCols; ++c) acc[c] = 0.0f;
                bool more = true;
                for (long long p0 = 0; more; p0 += kFoldLoads) {                  // wave-uniform
                    float r[kFoldLoads][kCols];
                    bool there[kFoldLoads];
#pragma unroll
                    for (int t = 0; t < kFoldLoads; ++t) {
                        const long long q = gc::chunk_start(q0, p0 + t, C);
                        there[t] = q < n_sorted && keys[q] == dest;
                        const float* row = scratch + (size_t)gc::slot_of(q, p0 + t, C) * W;
#pragma unroll
                        for (int c = 0; c < kCols; ++c)
                            r[t][c] = there[t] && f0 + 64 * c + lane < W ? row[f0 + 64 * c + lane] : 0.0f;
                    }
#pragma unroll
                    for (int t = 0; t < kFoldLoads; ++t) {
                        more = more && there[t];                                  // the chunks end at the first that is not there
                        if (more) {
#pragma unroll
                            for (int c = 0; c < kCols; ++c) acc[c] += r[t][c];
                        }
                    }
                }
#pragma unroll
                for (int c = 0; c < kCols; ++c)
                    if (f0 + 64 * c + lane < W) out[f0 + 64 * c + lane] = acc[c];
            }
        }
    }
}

// What a chunked entry point takes beyond its unchunked twin; a body that serves both takes a pointer to one, null for the twin.
struct Chunking { int32_t chunk; float* d_scratch; int64_t scratch_bytes; };

// The checks the three chunked entry points share: the chunk length and the caller's scratch.
int chunk_check(const char* where, const Chunking& c, int64_t n_sorted, int32_t width)
{
    if (!gp_gather_chunk::chunk_ok(c.chunk)) return fail(GP_ERR_INVALID_ARG, where, "chunk is not a power of two in [64, 4096]");
    const int64_t need = n_sorted > 0 && width > 0 ? gp_gather_chunk::scratch_bytes(n_sorted, c.chunk, width) : 0;
    if (c.scratch_bytes < need) return fail(GP_ERR_INVALID_ARG, where, "the scratch is smaller than GP_GATHER_CHUNK_SCRATCH_BYTES");
    if (need > 0 && !c.d_scratch) return fail(GP_ERR_NULL, where, "the scratch pointer is NULL");
    return GP_OK;
}

// Both launches, on the grid of gather_sum_kernel.
template <class Op>
int gather_chunked(const Op& op, const char* chunk_name, const int64_t* d_order, const int64_t* d_sorted_keys, int64_t n_sorted,
                   int64_t n_dest, int W, int chunk, float* dst, float* scratch, hipStream_t s)
{
    hipLaunchKernelGGL(gather_chunk_kernel<Op>, dim3(gather_grid(n_sorted)), dim3(kGather), 0, s, op, (const long long*)d_order,
                       (const long long*)d_sorted_keys, (long long)n_sorted, (long long)n_dest, W, chunk, dst, scratch);
    if (const int rc = launch_status(chunk_name)) return rc;
    hipLaunchKernelGGL(gather_fold_kernel, dim3(gather_grid(n_sorted)), dim3(kGather), 0, s, (const long long*)d_sorted_keys,
                       (long long)n_sorted, (long long)n_dest, W, chunk, (const float*)scratch, dst);
    return launch_status("gather_fold_kernel");
}

}  // namespace
