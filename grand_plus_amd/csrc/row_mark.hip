// row_mark.hip -- DESIGN §7u: a row list for MAG's atomic table gradient, so that the row-wise clip + Adam step of
// optim_rows.hip (§7t) serves the fast backward too.
//
// The atomic backward (mag_prop.hip, §7k) adds into a dense dW and keeps no list of the rows it added into; the
// deterministic one (mag_det.hip, §7o) has a list because it sorts its keys.  A sorted list of DISTINCT rows needs no sort:
//   row_mark_mag_kernel      a wave per slot of the batch, mag_keys_kernel's enumeration (slot_node of mag_stage.hpp); every
//                            in-range attribute id of the slot's bag sets its bit of a V-bit map with an atomic OR;
//   row_list_count_kernel    a workgroup per chunk of the map's words: the chunk's popcount into partials[blockIdx.x];
//   row_list_write_kernel    the same grid: the partials before the chunk, in order, are its offset; a scan per tile of 256
//                            words places every set bit; the words are cleared, the tail takes the sentinel V;
//   row_list_zero_kernel     a wave per list position: the row of `values` becomes 0.0f, for the atomics to add into.
// The layout -- word and bit of a row, the valid bits of the last word, the chunks, emit_word, tail and overflow -- is
// row_mark_layout.hpp's (HIP-free, held on the CPU by tests/native/row_mark_check.cpp).  The one atomic is the OR of the
// mark kernel, which is idempotent and commutative: the map, and so the list, is the same from run to run.  The count is
// decided in one launch and used in the next (the argument of gp_fit_snapshot): no workgroup waits for another.
#include "mag_stage.hpp"
#include "row_mark_layout.hpp"
#include "row_mark_abi.hpp"

#include <algorithm>

namespace {

constexpr int kBlock = gp_row_mark::kTile;                       // the compaction: a word per thread and tile
constexpr int kWaves = kBlock / 64;
constexpr int kMarkBlock = 256;                                  // the mark and zero kernels: a wave per slot / position

static_assert(gp_row_mark::kMaxChunks == GP_ROW_LIST_PARTIALS, "one partial per chunk");

__global__ void __launch_bounds__(kMarkBlock)
row_mark_mag_kernel(SlotArgs A, long long n_slots, unsigned* __restrict__ bitmap)
{
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * kMarkBlock + threadIdx.x) >> 6, n_waves = ((long long)gridDim.x * kMarkBlock) >> 6;
    for (long long e = wave; e < n_slots; e += n_waves) {                         // wave-uniform
        long long node;
        if (!slot_node(A, e, node)) continue;
        const long long lo = A.indptr[node], hi = A.indptr[node + 1];
        for (long long t = lo + lane; t < hi; t += 64) {
            const long long a = A.indices[t];
            if (a >= 0 && a < A.V) atomicOr(bitmap + gp_row_mark::word_of(a), gp_row_mark::bit_of(a));
        }
    }
}

__global__ void __launch_bounds__(kBlock)
row_list_count_kernel(const unsigned* __restrict__ bitmap, long long V, long long n_words, long long* __restrict__ partials)
{
    __shared__ long long lds[kWaves];
    const long long begin = gp_row_mark::chunk_begin(blockIdx.x, n_words, gridDim.x);
    const long long end = gp_row_mark::chunk_begin(blockIdx.x + 1ll, n_words, gridDim.x);
    long long n = 0;
    for (long long w = begin + threadIdx.x; w < end; w += kBlock) n += gp_row_mark::popcount(bitmap[w] & gp_row_mark::valid_mask(w, V));
    const long long s = block_sum<kWaves>(n, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ void __launch_bounds__(kBlock)
row_list_write_kernel(unsigned* __restrict__ bitmap, long long V, long long n_words, const long long* __restrict__ partials,
                      long long capacity, long long* __restrict__ keys, long long* __restrict__ count, int* __restrict__ flag)
{
    __shared__ long long lds[kWaves];
    __shared__ int s_wave[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the chunks before this one, and all of them: integers, every workgroup sums them in the same order
    long long before = 0, all = 0;
    for (int g = tid; g < (int)gridDim.x; g += kBlock) {
        const long long p = partials[g];
        all += p;
        if (g < (int)blockIdx.x) before += p;
    }
    long long carry = block_sum<kWaves>(before, lds);
    const long long total = block_sum<kWaves>(all, lds);

    const long long begin = gp_row_mark::chunk_begin(blockIdx.x, n_words, gridDim.x);
    const long long end = gp_row_mark::chunk_begin(blockIdx.x + 1ll, n_words, gridDim.x);
    for (long long w0 = begin; w0 < end; w0 += kBlock) {                           // workgroup-uniform
        const long long w = w0 + tid;
        const unsigned word = w < end ? bitmap[w] : 0u;
        const int n = gp_row_mark::popcount(word & gp_row_mark::valid_mask(w, V));
        int x = n;                                                                 // inclusive within the wave
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        __syncthreads();                                                           // the tile before has read s_wave
        if (lane == 63) s_wave[wave] = x;
        __syncthreads();
        long long off = carry;
        for (int v = 0; v < wave; ++v) off += s_wave[v];
        if (n) gp_row_mark::emit_word(word, w, off + x - n, V, capacity, keys);
        if (w < end && word) bitmap[w] = 0u;                                       // the map is all zero after the call
        for (int v = 0; v < kWaves; ++v) carry += s_wave[v];                       // every thread: the tile's count
    }
    const long long gtid = (long long)blockIdx.x * kBlock + tid, n_threads = (long long)gridDim.x * kBlock;
    for (long long j = gp_row_mark::tail_begin(total, capacity) + gtid; j < capacity; j += n_threads) keys[j] = V;
    if (gtid == 0) {
        *count = total;
        if (gp_row_mark::overflowed(total, capacity)) *flag = *flag | 1;           // one thread, a plain store
    }
}

template <bool kVec>
__global__ void __launch_bounds__(kMarkBlock)
row_list_zero_kernel(const long long* __restrict__ keys, long long capacity, long long V, int H, float* __restrict__ values)
{
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * kMarkBlock + threadIdx.x) >> 6, n_waves = ((long long)gridDim.x * kMarkBlock) >> 6;
    for (long long i = wave; i < capacity; i += n_waves) {                        // wave-uniform
        const long long key = keys[i];
        if (key >= V) break;                                                       // ascending: the sentinels follow
        if (key < 0) continue;
        float* row = values + key * H;
        if (kVec) {
            for (int h = lane * 4; h < H; h += 256) *reinterpret_cast<float4*>(row + h) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        } else {
            for (int h = lane; h < H; h += 64) row[h] = 0.0f;
        }
    }
}

int wave_grid(long long n)                                     // workgroups of kMarkBlock threads, a wave per item, capped
{
    const long long g = (n + kMarkBlock / 64 - 1) / (kMarkBlock / 64);
    return (int)std::min<long long>(kGridCap, std::max<long long>(g, 1));
}

}  // namespace

extern "C" {

int gp_row_mark_mag(int device, int64_t n_vocab, const int64_t* d_attr_indptr, const int32_t* d_attr_indices, int64_t n_nodes,
                    const int32_t* d_col, const int32_t* d_filled, int64_t n_rows, int32_t K, const int32_t* d_batch_rows,
                    int32_t n_batch, int32_t* d_bitmap, void* stream)
{
    const char* where = "gp_row_mark_mag";
    if (n_vocab < 1 || n_nodes < 0 || n_rows < 0 || K < 1 || K > GP_MAX_K || n_batch < 0)
        return fail(GP_ERR_INVALID_ARG, where, "bad size or K outside [1, 1024]");
    if ((int64_t)n_batch * K >= (1ll << 31)) return fail(GP_ERR_INVALID_ARG, where, "n_batch * K >= 2^31");
    if (!d_attr_indptr || !d_attr_indices || !d_col || !d_bitmap) return fail(GP_ERR_NULL, where, "a device pointer is NULL");
    if (n_batch == 0) return GP_OK;
    if (const int rc = set_device(device, where)) return rc;
    const long long n_slots = (long long)n_batch * K;
    const SlotArgs A = {(const long long*)d_attr_indptr, d_attr_indices, n_nodes, n_vocab, d_col, d_filled, n_rows, K, d_batch_rows};
    hipLaunchKernelGGL(row_mark_mag_kernel, dim3(wave_grid(n_slots)), dim3(kMarkBlock), 0, (hipStream_t)stream, A, n_slots,
                       reinterpret_cast<unsigned*>(d_bitmap));
    return launch_status("row_mark_mag_kernel");
}

int gp_row_list_compact(int device, int64_t n_vocab, int32_t* d_bitmap, int64_t capacity, int64_t* d_keys, int64_t* d_count,
                        int64_t* d_partials, int32_t* d_flag, void* stream)
{
    const char* where = "gp_row_list_compact";
    if (n_vocab < 1 || capacity < 1) return fail(GP_ERR_INVALID_ARG, where, "n_vocab < 1 or capacity < 1");
    if (!d_bitmap || !d_keys || !d_count || !d_partials || !d_flag) return fail(GP_ERR_NULL, where, "a device pointer is NULL");
    if (const int rc = set_device(device, where)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const long long n_words = gp_row_mark::words(n_vocab);
    const dim3 grid((int)gp_row_mark::chunks(n_words)), block(kBlock);
    unsigned* bitmap = reinterpret_cast<unsigned*>(d_bitmap);
    hipLaunchKernelGGL(row_list_count_kernel, grid, block, 0, s, (const unsigned*)bitmap, (long long)n_vocab, n_words,
                       (long long*)d_partials);
    if (const int rc = launch_status("row_list_count_kernel")) return rc;
    hipLaunchKernelGGL(row_list_write_kernel, grid, block, 0, s, bitmap, (long long)n_vocab, n_words, (const long long*)d_partials,
                       (long long)capacity, (long long*)d_keys, (long long*)d_count, d_flag);
    return launch_status("row_list_write_kernel");
}

int gp_row_list_zero(int device, const int64_t* d_keys, int64_t capacity, int64_t n_vocab, int32_t dim, float* d_values,
                     void* stream)
{
    const char* where = "gp_row_list_zero";
    if (capacity < 1 || n_vocab < 1 || dim < 1) return fail(GP_ERR_INVALID_ARG, where, "capacity < 1, n_vocab < 1 or dim < 1");
    if (n_vocab > INT64_MAX / dim) return fail(GP_ERR_INVALID_ARG, where, "n_vocab * dim does not fit 63 bits");
    if (!d_keys || !d_values) return fail(GP_ERR_NULL, where, "d_keys or d_values is NULL");
    if (const int rc = set_device(device, where)) return rc;
    const dim3 grid(wave_grid(capacity)), block(kMarkBlock);
    const long long* keys = (const long long*)d_keys;
    if ((dim & 3) == 0 && ((uintptr_t)d_values & 15) == 0)
        hipLaunchKernelGGL(row_list_zero_kernel<true>, grid, block, 0, (hipStream_t)stream, keys, (long long)capacity, (long long)n_vocab, dim, d_values);
    else
        hipLaunchKernelGGL(row_list_zero_kernel<false>, grid, block, 0, (hipStream_t)stream, keys, (long long)capacity, (long long)n_vocab, dim, d_values);
    return launch_status("row_list_zero_kernel");
}

}  // extern "C"
