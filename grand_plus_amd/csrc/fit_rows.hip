// fit_rows.hip -- DESIGN §7v: the best-weights snapshot of an embedding table that copies only the rows that changed since
// the last snapshot (fit_rows_abi.hpp).
//
// gp_fit_snapshot (fit.hip, §7n) copies a tensor whole.  Under the lazy table step (§7t) a step changes only the rows its
// batch's bags name, and the backward already holds their list; so
//   fit_rows_mark_kernel      a thread per key of that list: an in-range key that differs from the key before it sets its
//                             bit of a V-bit map with an atomic OR -- the one atomic here, idempotent and commutative, so the
//                             map is the same from run to run;
//   fit_rows_snapshot_kernel  when the rule said so (gp_fit_track::copy_now, decided by a launch before this one, the
//                             argument of gp_fit_snapshot), a wave per word of the map: the set rows are copied from the
//                             table into its snapshot as bits, then the word is cleared.  Plain C++ loads and stores.
// The map's layout is row_mark_layout.hpp's; which wave owns which word, and which lane copies which unit of which row,
// is fit_rows_layout.hpp's (HIP-free, held on the CPU by tests/native/fit_rows_check.cpp).
#include "gp_common.hpp"

#include "fit_rows_layout.hpp"
#include "fit_rows_abi.hpp"

#include <algorithm>

namespace {

constexpr int kBlock = gp_fit_rows::kWaves * gp_fit_rows::kLanes;
constexpr int kMaxGrid = 2048;                    // workgroups of either kernel; the rest is walked grid-stride

__global__ void __launch_bounds__(kBlock)
fit_rows_mark_kernel(const long long* __restrict__ keys, long long n_keys, long long V, unsigned* __restrict__ dirty)
{
    const long long n_threads = (long long)gridDim.x * kBlock;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n_keys; i += n_threads) {
        const long long key = keys[i];
        if (key < 0 || key >= V) continue;                                         // the sentinel tail, a stray key: no address
        if (i > 0 && keys[i - 1] == key) continue;                                 // a run of one row: its first key marks
        atomicOr(dirty + gp_row_mark::word_of(key), gp_row_mark::bit_of(key));
    }
}

// T: uint4 (per_row = dim / 4) or unsigned (per_row = dim).
template <class T>
__global__ void __launch_bounds__(kBlock)
fit_rows_snapshot_kernel(const gp_fit_track* __restrict__ tr, const T* __restrict__ src, T* __restrict__ dst, long long V,
                         long long per_row, int g, long long n_words, unsigned* __restrict__ dirty)
{
    if (tr->copy_now == 0) return;
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * kBlock + threadIdx.x) >> 6, n_waves = ((long long)gridDim.x * kBlock) >> 6;
    const long long n_trips = gp_fit_rows::trips(n_words, n_waves);
    const int first = gp_fit_rows::lane_first(lane, g), step = 1 << g;
    for (long long trip = 0; trip < n_trips; ++trip) {                             // wave-uniform
        const long long w = gp_fit_rows::owned_word(wave, trip, n_waves);
        if (w >= n_words) break;
        const unsigned word = dirty[w];                                            // this wave's word alone
        if (word == 0u) continue;
        const unsigned bits = gp_fit_rows::live_bits(word, w, V);
        const int n = gp_row_mark::popcount(bits), n_passes = gp_fit_rows::passes(n, g);
        for (int pass = 0; pass < n_passes; ++pass) {
            const int k = gp_fit_rows::lane_slot(lane, pass, g);
            if (k < n) {
                const long long at = gp_fit_rows::nth_row(bits, w, k) * per_row;
                for (long long j = first; j < per_row; j += step) dst[at + j] = src[at + j];
            }
        }
        if (lane == 0) dirty[w] = 0u;
    }
}

bool misaligned(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }

}  // namespace

extern "C" {

int gp_fit_rows_mark(int device, const int64_t* d_keys, int64_t n_keys, int64_t n_vocab, int32_t* d_dirty, void* stream)
{
    const char* where = "gp_fit_rows_mark";
    if (n_vocab < 1 || n_keys < 0) return fail(GP_ERR_INVALID_ARG, where, "n_vocab < 1 or n_keys < 0");
    if (!d_keys || !d_dirty) return fail(GP_ERR_NULL, where, "d_keys or d_dirty is NULL");
    if (misaligned(d_keys, 3) || misaligned(d_dirty, 3)) return fail(GP_ERR_INVALID_ARG, where, "a pointer is not 4-byte aligned");
    if (n_keys == 0) return GP_OK;
    if (const int rc = set_device(device, where)) return rc;
    const long long blocks = ((long long)n_keys + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(fit_rows_mark_kernel, dim3((unsigned)std::min<long long>(blocks, kMaxGrid)), dim3(kBlock), 0, (hipStream_t)stream,
                       (const long long*)d_keys, (long long)n_keys, (long long)n_vocab, reinterpret_cast<unsigned*>(d_dirty));
    return launch_status("fit_rows_mark_kernel");
}

int gp_fit_rows_snapshot(int device, const gp_fit_track* d_track, const void* d_src, void* d_dst, int64_t n_vocab, int32_t dim,
                         int32_t* d_dirty, void* stream)
{
    const char* where = "gp_fit_rows_snapshot";
    if (n_vocab < 1 || dim < 1) return fail(GP_ERR_INVALID_ARG, where, "n_vocab < 1 or dim < 1");
    if (n_vocab > INT64_MAX / dim) return fail(GP_ERR_INVALID_ARG, where, "n_vocab * dim does not fit 63 bits");
    if (!d_track || !d_src || !d_dst || !d_dirty) return fail(GP_ERR_NULL, where, "the track, d_src, d_dst or d_dirty is NULL");
    if (misaligned(d_track, 3) || misaligned(d_src, 3) || misaligned(d_dst, 3) || misaligned(d_dirty, 3))
        return fail(GP_ERR_INVALID_ARG, where, "a pointer is not 4-byte aligned");
    if (const int rc = set_device(device, where)) return rc;
    const long long n_words = gp_row_mark::words(n_vocab);
    const dim3 grid((unsigned)gp_fit_rows::grid(n_words, kMaxGrid)), block(kBlock);
    unsigned* dirty = reinterpret_cast<unsigned*>(d_dirty);
    if ((dim & 3) == 0 && !misaligned(d_src, 15) && !misaligned(d_dst, 15)) {
        const long long per_row = dim / 4;
        hipLaunchKernelGGL(fit_rows_snapshot_kernel<uint4>, grid, block, 0, (hipStream_t)stream, d_track, (const uint4*)d_src, (uint4*)d_dst,
                           (long long)n_vocab, per_row, gp_fit_rows::group_log2(per_row), n_words, dirty);
    } else {
        const long long per_row = dim;
        hipLaunchKernelGGL(fit_rows_snapshot_kernel<unsigned>, grid, block, 0, (hipStream_t)stream, d_track, (const unsigned*)d_src,
                           (unsigned*)d_dst, (long long)n_vocab, per_row, gp_fit_rows::group_log2(per_row), n_words, dirty);
    }
    return launch_status("fit_rows_snapshot_kernel");
}

}  // extern "C"
