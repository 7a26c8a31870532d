// mag_det.hip -- DESIGN §7o: the gradient of MAG's fused front end (mag_prop.hip, §7k) to the embedding table without
// atomics, so that it is bitwise the same run to run, and without a host read, so that a whole MAG step can be captured.
// Sort-then-gather as in scatter_det.hip (§7i), but here the entries of a call are not known to the host: a slot of the
// batch contributes one entry per element of its node's bag, and how many that is stands in device memory alone.  So
//   gp_mag_det_keys                 counts the entries per slot, scans the counts (slot_base) and writes every entry's
//                                   attribute id into a key buffer of a size the caller fixed beforehand (max_entries);
//                                   the tail carries the sentinel V, and an overflow sets a flag instead of writing;
//   the caller                      sorts the keys with a stable sort (plumbing, torch.sort);
//   gp_mag_prop_rows_backward_det   writes U[e, :] = the gradient that reaches slot e's embedding, once per slot, then
//                                   gather_sum_kernel<MagOp> sums U[e_j, :] * d_j per table row in entry order.
// The order contract is stated in mag_det_abi.hpp; the slot / entry arithmetic is mag_det_layout.hpp's (HIP-free, held
// on the CPU by tests/native/mag_det_check.cpp).  A slot is present, weighted and normalised as the forward has it:
// MagArgs, stage_row and the workgroup shape are mag_stage.hpp's, sample_weight, row_len and the two denominators
// dropnode.hpp's -- the lines mag_prop.hip calls.
#include "mag_stage.hpp"
#include "gather_sum.hpp"
#include "mag_det_layout.hpp"
#include "mag_det_abi.hpp"
#include "gather_chunk.hpp"
#include "gather_chunk_abi.hpp"

#include <algorithm>

namespace {

constexpr int kBlock = 256;           // the length and key kernels
constexpr int kScan = 1024;           // the scan: one workgroup

// SlotArgs and slot_node -- what finds a slot's node -- are mag_stage.hpp's: row_mark.hip (§7u) enumerates the same slots.

// ---- 1. slot_base[e] = len_e
__global__ void __launch_bounds__(kBlock)
mag_slot_len_kernel(SlotArgs A, long long n_slots, long long* __restrict__ slot_base)
{
    for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < n_slots; e += (long long)gridDim.x * kBlock) {
        long long node, len = 0;
        if (slot_node(A, e, node)) len = A.indptr[node + 1] - A.indptr[node];
        slot_base[e] = len > 0 ? len : 0;                                          // the forward's loop runs lo .. hi - 1
    }
}

// ---- 2. slot_base[0 .. n_slots] = the exclusive prefix sum of the lengths, in place; one workgroup walks the slots
__global__ void __launch_bounds__(kScan)
mag_slot_scan_kernel(long long n_slots, long long* __restrict__ slot_base)
{
    __shared__ long long s_wave[kScan / 64];
    __shared__ long long s_carry;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (long long c0 = 0; c0 < n_slots; c0 += kScan) {                           // workgroup-uniform
        const long long i = c0 + threadIdx.x;
        const long long v = i < n_slots ? slot_base[i] : 0;
        long long x = v;                                                           // inclusive within the wave
        for (int o = 1; o < 64; o <<= 1) {
            const long long y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        if (lane == 63) s_wave[wave] = x;
        __syncthreads();
        long long off = s_carry;
        for (int w = 0; w < wave; ++w) off += s_wave[w];
        if (i < n_slots) slot_base[i] = off + x - v;
        __syncthreads();
        if (threadIdx.x == kScan - 1) s_carry = off + x;
        __syncthreads();
    }
    if (threadIdx.x == 0) slot_base[n_slots] = s_carry;
}

// ---- 3. the keys: a wave per slot; then every thread helps with the tail
__global__ void __launch_bounds__(kBlock)
mag_keys_kernel(SlotArgs A, long long n_slots, const long long* __restrict__ slot_base, long long max_entries,
                long long* __restrict__ keys, int* __restrict__ flag)
{
    const int lane = threadIdx.x & 63;
    const long long tid = (long long)blockIdx.x * kBlock + threadIdx.x, n_threads = (long long)gridDim.x * kBlock;
    for (long long e = tid >> 6; e < n_slots; e += n_threads >> 6) {              // wave-uniform
        const long long base = slot_base[e], len = slot_base[e + 1] - base;
        long long node;
        if (len <= 0 || !slot_node(A, e, node)) continue;
        const long long lo = A.indptr[node];
        for (long long t = lane; t < len; t += 64) {
            const long long j = base + t;
            if (j >= max_entries) break;                                           // written nowhere: the flag says so
            const long long a = A.indices[lo + t];
            keys[j] = a >= 0 && a < A.V ? a : A.V;
        }
    }
    const long long total = slot_base[n_slots];
    for (long long j = gp_mag_det::tail_begin(total, max_entries) + tid; j < max_entries; j += n_threads) keys[j] = A.V;
    if (tid == 0 && gp_mag_det::overflowed(total, max_entries)) *flag = *flag | 1;    // one thread, a plain store
}

// ---- U[e, :] of every slot that exists, and inv[s, b].  The staging, the two denominators and the expression of c are
// mag_prop_rows_backward_kernel's (mag_prop.hip); where that adds c * inv_den * d_t to dW[a_t] with an atomic per entry,
// this writes c * inv_den once per slot.  LDS: s_col[K] s_inv[16] s_w[nsc][K].  When the S weight rows do not fit one
// stage (K * S large), U holds the running c between the chunks: the sum stays the one sequential sum over s.
__global__ void __launch_bounds__(kMaxWaves * 64)
mag_slot_grad_kernel(const float* __restrict__ grad_out, MagArgs A, float* __restrict__ U, float* __restrict__ inv)
{
    extern __shared__ float smem[];
    constexpr int MS = kMaxSamples;
    const int K = A.K, H = A.H, nsc = A.nsc;
    int* s_col = reinterpret_cast<int*>(smem);
    float* s_inv = smem + K;
    float* s_w = s_inv + kMaxSamples;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    const float scale_node = inv_keep(A.p_node);
    const size_t g_stride = (size_t)A.B * H;
    const u64 seed = call_seed(A);
    for (int b = blockIdx.x; b < A.B; b += gridDim.x) {
        const long long row = A.batch_rows ? (long long)A.batch_rows[b] : (long long)b;
        if (row < 0 || row >= A.n_rows) {                                         // workgroup-uniform: no slot of b exists
            if (threadIdx.x < A.S) inv[(size_t)threadIdx.x * A.B + b] = 0.0f;
            continue;
        }
        const int n = A.filled ? max(0, min(A.filled[row], K)) : K;             // as the forward: not row_len
        u64 any_mask = 0;                     // bit i: this wave's i-th slot is kept in some sample (at most 64 slots a wave)
        for (int s0 = 0; s0 < A.S; s0 += nsc) {
            const int ns = min(nsc, A.S - s0);
            const bool first = s0 == 0, last = s0 + ns >= A.S;
            __syncthreads();
            stage_row(A, seed, row, n, s0, ns, scale_node, s_col, nullptr, s_w, nullptr);
            __syncthreads();
            if (threadIdx.x < ns) {
                float den = 0.0f;
                for (int k = 0; k < n; ++k) den += s_w[threadIdx.x * K + k];      // the forward's order
                s_inv[threadIdx.x] = inv_den_rows(den);
                inv[(size_t)(s0 + threadIdx.x) * A.B + b] = s_inv[threadIdx.x];
            }
            __syncthreads();
            for (int hc = 0; hc < H; hc += 64) {
                const int h = hc + lane;
                const bool h_live = h < H;
                float gs[MS];
#pragma unroll
                for (int s = 0; s < MS; ++s)
                    gs[s] = s < ns && h_live ? grad_out[(size_t)(s0 + s) * g_stride + (size_t)b * H + h] * s_inv[s] : 0.0f;
                int slot = 0;
                for (int k = wave; k < n; k += n_waves, ++slot) {                  // wave-uniform
                    const long long node = s_col[k];
                    if (node < 0 || node >= A.N) continue;                        // the slot does not exist
                    bool any = false;
                    for (int s = 0; s < ns; ++s) any |= s_w[s * K + k] != 0.0f;
                    if (any) any_mask |= 1ull << slot;
                    float* u = U + ((size_t)b * K + k) * H;
                    float c = first || !h_live ? 0.0f : u[h];
#pragma unroll
                    for (int s = 0; s < MS; ++s) {
                        const float ws = s < ns ? s_w[s * K + k] : 0.0f;
                        const float x = gs[s] * ws;
                        if (s < ns) c += x;                                       // s ascending, from 0.0f
                    }
                    if (last) {
                        float cd = 0.0f;                                          // dropped in every sample: U = 0, the bag is not read
                        if ((any_mask >> slot) & 1) {
                            const long long lo = A.indptr[node], hi = A.indptr[node + 1];
                            float den = 0.0f;
                            for (long long c0 = lo; c0 < hi; c0 += 64) {          // sequentially in t, as the forward
                                const float my_d = c0 + lane < hi ? A.data[c0 + lane] : 0.0f;
                                const int cnt = (int)(hi - c0 < 64 ? hi - c0 : 64);
                                for (int t = 0; t < cnt; ++t) den += __shfl(my_d, t);
                            }
                            cd = c * inv_den_bag(den);
                        }
                        c = cd;
                    }
                    if (h_live) u[h] = c;
                }
            }
        }
    }
}

// ---- what one sorted position contributes (the Op of gather_sum_kernel: scatter_det.hip describes load and add)
struct MagOp {
    const float* U; int H; SlotArgs A; const float* data; const long long* slot_base; long long n_slots, max_entries;

    struct Entry { long long e; float d; int live; };

    __device__ __forceinline__ Entry load(const long long* __restrict__ order, long long i, bool want, long long key) const
    {
        Entry E;
        E.e = 0; E.d = 0.0f; E.live = 0;
        if (!want) return E;
        const long long j = order[i];
        if (j < 0 || j >= gp_mag_det::live_entries(slot_base[n_slots], max_entries)) return E;
        const long long e = gp_mag_det::slot_of(slot_base, n_slots, j);
        if (e >= n_slots) return E;
        const long long t = j - slot_base[e];
        long long node;
        if (!slot_node(A, e, node)) return E;
        const long long lo = A.indptr[node], hi = A.indptr[node + 1];
        if (t < 0 || t >= hi - lo || (long long)A.indices[lo + t] != key) return E;
        E.e = e; E.d = data[lo + t]; E.live = 1;
        return E;
    }

    __device__ __forceinline__ void add(const Entry& E, int u, int f, float (&acc)[kCols]) const
    {
        if (!__shfl(E.live, u)) return;                              // wave-uniform
        const float* up = U + (size_t)__shfl(E.e, u) * H;
        const float d = __shfl(E.d, u);
#pragma unroll
        for (int c = 0; c < kCols; ++c)
            if (f + 64 * c < H) acc[c] += up[f + 64 * c] * d;
    }
};

int slots_check(const char* where, int32_t K, int32_t n_batch, int64_t max_entries)
{
    if (max_entries < 1 || (K >= 1 && n_batch >= 0 && (int64_t)n_batch * K >= (1ll << 31)))
        return fail(GP_ERR_INVALID_ARG, where, "max_entries < 1 or n_batch * K >= 2^31");
    return GP_OK;
}

// gp_mag_prop_rows_backward_det and its chunked twin: the checks, U and inv and the Op are the same, the gather is
// gather_sum_kernel, or with a Chunking gather_chunk.hpp's.  where: the entry point that was called.
int mag_backward_det(const char* where, int device, const float* d_grad_out, int64_t n_vocab, int32_t dim,
                     const int64_t* d_attr_indptr, const int32_t* d_attr_indices, const float* d_attr_data, int64_t n_nodes,
                     const int32_t* d_col, const double* d_val, const int32_t* d_filled, int64_t n_rows, int32_t K,
                     const int32_t* d_batch_rows, int32_t n_batch, int32_t n_samples, float dropnode_rate, float input_droprate,
                     int training, uint64_t seed, const uint8_t* d_keep, int64_t keep_stride, const int64_t* d_slot_base,
                     const int64_t* d_order, const int64_t* d_sorted_keys, int64_t max_entries, float* d_slot_grad, float* d_inv,
                     float* d_dW, const Chunking* chunking, void* stream)
{
    if (const int rc = mag_check(where, n_vocab, dim, n_nodes, n_rows, K, n_batch, n_samples, dropnode_rate, input_droprate,
                                 d_keep, keep_stride)) return rc;
    if (training && input_droprate > 0.0f)
        return fail(GP_ERR_INVALID_ARG, where, "input dropout is not supported by the deterministic backward (DESIGN §9)");
    if (const int rc = slots_check(where, K, n_batch, max_entries)) return rc;
    if (chunking)
        if (const int rc = chunk_check(where, *chunking, n_batch == 0 ? 0 : max_entries, dim)) return rc;
    if (n_batch == 0) return GP_OK;
    if (!d_grad_out || !d_attr_indptr || !d_attr_indices || !d_attr_data || !d_col || !d_val || !d_slot_base || !d_order ||
        !d_sorted_keys || !d_slot_grad || !d_inv || !d_dW)
        return fail(GP_ERR_NULL, where, "a device pointer is NULL");
    if (const int rc = set_device(device, where)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int n_waves = waves_for(K);
    const int nsc = std::min<int>(n_samples, (kLdsFloats - K - kMaxSamples) / K);
    const size_t lds = (size_t)(K + kMaxSamples + nsc * K) * 4;
    const MagArgs A = {n_vocab, dim, (const long long*)d_attr_indptr, d_attr_indices, d_attr_data, n_nodes, d_col, d_val, d_filled,
                       n_rows, K, d_batch_rows, n_batch, n_samples, nsc, dropnode_rate, 0.0f, training, (u64)seed,
                       d_keep, (long long)keep_stride};
    hipLaunchKernelGGL(mag_slot_grad_kernel, dim3(std::min<int>(n_batch, kGridCap)), dim3(n_waves * 64), lds, s, d_grad_out, A,
                       d_slot_grad, d_inv);
    if (const int rc = launch_status("mag_slot_grad_kernel")) return rc;
    const MagOp op = {d_slot_grad, dim, {(const long long*)d_attr_indptr, d_attr_indices, n_nodes, n_vocab, d_col, d_filled, n_rows, K,
                                         d_batch_rows},
                      d_attr_data, (const long long*)d_slot_base, (long long)n_batch * K, (long long)max_entries};
    if (!chunking) {
        hipLaunchKernelGGL(gather_sum_kernel<MagOp>, dim3(gather_grid(max_entries)), dim3(kGather), 0, s, op, (const long long*)d_order,
                           (const long long*)d_sorted_keys, (long long)max_entries, (long long)n_vocab, dim, d_dW);
        return launch_status("gather_sum_kernel<MagOp>");
    }
    return gather_chunked(op, "gather_chunk_kernel<MagOp>", d_order, d_sorted_keys, max_entries, n_vocab, dim, chunking->chunk, d_dW,
                          chunking->d_scratch, s);
}

}  // namespace

extern "C" {

int gp_mag_det_keys(int device, int64_t n_vocab, const int64_t* d_attr_indptr, const int32_t* d_attr_indices, int64_t n_nodes,
                    const int32_t* d_col, const int32_t* d_filled, int64_t n_rows, int32_t K, const int32_t* d_batch_rows,
                    int32_t n_batch, int64_t max_entries, int64_t* d_slot_base, int64_t* d_keys, int32_t* d_flag, void* stream)
{
    const char* where = "gp_mag_det_keys";
    if (n_vocab < 1 || n_nodes < 0 || n_rows < 0 || K < 1 || K > GP_MAX_K || n_batch < 0)
        return fail(GP_ERR_INVALID_ARG, where, "bad size or K outside [1, 1024]");
    if (const int rc = slots_check(where, K, n_batch, max_entries)) return rc;
    if (n_batch == 0) return GP_OK;
    if (!d_attr_indptr || !d_attr_indices || !d_col || !d_slot_base || !d_keys || !d_flag)
        return fail(GP_ERR_NULL, where, "a device pointer is NULL");
    if (const int rc = set_device(device, where)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const long long n_slots = (long long)n_batch * K;
    const SlotArgs A = {(const long long*)d_attr_indptr, d_attr_indices, n_nodes, n_vocab, d_col, d_filled, n_rows, K, d_batch_rows};
    long long* base = (long long*)d_slot_base;
    hipLaunchKernelGGL(mag_slot_len_kernel, dim3((int)std::min<long long>(kGridCap, (n_slots + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                       A, n_slots, base);
    if (const int rc = launch_status("mag_slot_len_kernel")) return rc;
    hipLaunchKernelGGL(mag_slot_scan_kernel, dim3(1), dim3(kScan), 0, s, n_slots, base);
    if (const int rc = launch_status("mag_slot_scan_kernel")) return rc;
    const long long waves = kBlock / 64;
    hipLaunchKernelGGL(mag_keys_kernel, dim3((int)std::min<long long>(kGridCap, (n_slots + waves - 1) / waves)), dim3(kBlock), 0, s,
                       A, n_slots, (const long long*)base, (long long)max_entries, (long long*)d_keys, d_flag);
    return launch_status("mag_keys_kernel");
}

int gp_mag_prop_rows_backward_det(int device, const float* d_grad_out, int64_t n_vocab, int32_t dim,
                                  const int64_t* d_attr_indptr, const int32_t* d_attr_indices, const float* d_attr_data,
                                  int64_t n_nodes, const int32_t* d_col, const double* d_val, const int32_t* d_filled,
                                  int64_t n_rows, int32_t K, const int32_t* d_batch_rows, int32_t n_batch,
                                  int32_t n_samples, float dropnode_rate, float input_droprate, int training,
                                  uint64_t seed, const uint8_t* d_keep, int64_t keep_stride, const int64_t* d_slot_base,
                                  const int64_t* d_order, const int64_t* d_sorted_keys, int64_t max_entries,
                                  float* d_slot_grad, float* d_inv, float* d_dW, void* stream)
{
    return mag_backward_det("gp_mag_prop_rows_backward_det", device, d_grad_out, n_vocab, dim, d_attr_indptr, d_attr_indices,
                            d_attr_data, n_nodes, d_col, d_val, d_filled, n_rows, K, d_batch_rows, n_batch, n_samples, dropnode_rate,
                            input_droprate, training, seed, d_keep, keep_stride, d_slot_base, d_order, d_sorted_keys, max_entries,
                            d_slot_grad, d_inv, d_dW, nullptr, stream);
}

// The chunked twin (gather_chunk_abi.hpp states its contract): U and inv as above, the gather cut into chunks of
// `chunk` sorted positions by gather_chunk.hpp.
int gp_mag_prop_rows_backward_det_chunked(int device, const float* d_grad_out, int64_t n_vocab, int32_t dim,
                                          const int64_t* d_attr_indptr, const int32_t* d_attr_indices, const float* d_attr_data,
                                          int64_t n_nodes, const int32_t* d_col, const double* d_val, const int32_t* d_filled,
                                          int64_t n_rows, int32_t K, const int32_t* d_batch_rows, int32_t n_batch,
                                          int32_t n_samples, float dropnode_rate, float input_droprate, int training,
                                          uint64_t seed, const uint8_t* d_keep, int64_t keep_stride, const int64_t* d_slot_base,
                                          const int64_t* d_order, const int64_t* d_sorted_keys, int64_t max_entries,
                                          float* d_slot_grad, float* d_inv, float* d_dW, int32_t chunk, float* d_scratch,
                                          int64_t scratch_bytes, void* stream)
{
    const Chunking chunking = {chunk, d_scratch, scratch_bytes};
    return mag_backward_det("gp_mag_prop_rows_backward_det_chunked", device, d_grad_out, n_vocab, dim, d_attr_indptr, d_attr_indices,
                            d_attr_data, n_nodes, d_col, d_val, d_filled, n_rows, K, d_batch_rows, n_batch, n_samples, dropnode_rate,
                            input_droprate, training, seed, d_keep, keep_stride, d_slot_base, d_order, d_sorted_keys, max_entries,
                            d_slot_grad, d_inv, d_dW, &chunking, stream);
}

}  // extern "C"
