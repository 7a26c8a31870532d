// mag_drop.hip -- DESIGN §7y: the deterministic gradient of MAG's front end to the embedding table WITH input dropout.
// mag_det.hip (§7o) sums the samples into one U[e, :] per slot and gathers U[e_j, :] * d_j per table row; with input dropout
// every (sample, bag position, column) has a mask factor of its own, so the samples must reach the gather apart:
//   mag_slot_grad_samples_kernel   writes U[s, e, :] = the gradient that reaches slot e's embedding in sample s, and inv[s, b];
//   the gather                     sums, per entry, the samples' U[s, e_j, :] * d_j under their masks, and per table row the
//                                  entries in entry order: gather_sum_kernel, or with a chunk gather_chunk.hpp's, over an Op
//                                  that mag_prop.hip keeps next to GP_MAG_SLOT_SEED's one definition (mag_drop_gather.hpp).
// Keys, slot_base, the sort and the overflow flag are gp_mag_det_keys' (mag_det.hip).  The order contract is stated in
// mag_drop_abi.hpp.  A slot is present, weighted and normalised as the forward has it: MagArgs, stage_row, call_seed and
// the workgroup shape are mag_stage.hpp's, sample_weight, row_len and the two denominators dropnode.hpp's -- the lines
// mag_prop.hip and mag_det.hip call.  No atomics, no host read: every launch can be captured.
#include "mag_stage.hpp"
#include "gather_chunk_layout.hpp"
#include "mag_drop_abi.hpp"
#include "mag_drop_gather.hpp"

#include <algorithm>

namespace {

// ---- U[s, e, :] of every slot that exists and every sample, and inv[s, b].  mag_det.hip's mag_slot_grad_kernel with the
// samples kept apart: where that adds x_s = (g[s, b] * inv_s) * w'_s over s and scales the sum by the bag's inv_den, this
// stores x_s * inv_den per sample (0 where w'_s == 0) -- mag_prop_rows_backward_kernel's cs[s].  A chunk of samples is
// complete in itself, so nothing is carried between the LDS stages.  LDS: s_col[K] s_inv[16] s_w[nsc][K].
__global__ void __launch_bounds__(kMaxWaves * 64)
mag_slot_grad_samples_kernel(const float* __restrict__ grad_out, MagArgs A, float* __restrict__ U, float* __restrict__ inv)
{
    extern __shared__ float smem[];
    const int K = A.K, H = A.H, nsc = A.nsc;
    int* s_col = reinterpret_cast<int*>(smem);
    float* s_inv = smem + K;
    float* s_w = s_inv + kMaxSamples;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    const float scale_node = inv_keep(A.p_node);
    const size_t g_stride = (size_t)A.B * H, u_stride = (size_t)A.B * K * H;
    const u64 seed = call_seed(A);
    for (int b = blockIdx.x; b < A.B; b += gridDim.x) {
        const long long row = A.batch_rows ? (long long)A.batch_rows[b] : (long long)b;
        if (row < 0 || row >= A.n_rows) {                                         // workgroup-uniform: no slot of b exists
            if (threadIdx.x < A.S) inv[(size_t)threadIdx.x * A.B + b] = 0.0f;
            continue;
        }
        const int n = A.filled ? max(0, min(A.filled[row], K)) : K;             // as the forward: not row_len
        for (int s0 = 0; s0 < A.S; s0 += nsc) {
            const int ns = min(nsc, A.S - s0);
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
            for (int k = wave; k < n; k += n_waves) {                             // wave-uniform
                const long long node = s_col[k];
                if (node < 0 || node >= A.N) continue;                            // the slot does not exist
                bool any = false;
                for (int s = 0; s < ns; ++s) any |= s_w[s * K + k] != 0.0f;
                float inv_den = 0.0f;                                             // dropped in every sample of the chunk: the bag is not read
                if (any) {
                    const long long lo = A.indptr[node], hi = A.indptr[node + 1];
                    float den = 0.0f;
                    for (long long c0 = lo; c0 < hi; c0 += 64) {                  // sequentially in t, as the forward
                        const float my_d = c0 + lane < hi ? A.data[c0 + lane] : 0.0f;
                        const int cnt = (int)(hi - c0 < 64 ? hi - c0 : 64);
                        for (int t = 0; t < cnt; ++t) den += __shfl(my_d, t);
                    }
                    inv_den = inv_den_bag(den);
                }
                for (int hc = 0; hc < H; hc += 64) {
                    const int h = hc + lane;
                    if (h >= H) continue;
                    for (int s = 0; s < ns; ++s) {
                        const float ws = s_w[s * K + k];
                        const float x = (grad_out[(size_t)(s0 + s) * g_stride + (size_t)b * H + h] * s_inv[s]) * ws;
                        U[(size_t)(s0 + s) * u_stride + ((size_t)b * K + k) * H + h] = ws != 0.0f ? x * inv_den : 0.0f;
                    }
                }
            }
        }
    }
}

}  // namespace

extern "C" {

int gp_mag_prop_rows_backward_det_drop(int device, const float* d_grad_out, int64_t n_vocab, int32_t dim,
                                       const int64_t* d_attr_indptr, const int32_t* d_attr_indices, const float* d_attr_data,
                                       int64_t n_nodes, const int32_t* d_col, const double* d_val, const int32_t* d_filled,
                                       int64_t n_rows, int32_t K, const int32_t* d_batch_rows, int32_t n_batch,
                                       int32_t n_samples, float dropnode_rate, float input_droprate, int training,
                                       uint64_t seed, const uint64_t* d_seed, const uint8_t* d_keep, int64_t keep_stride,
                                       const int64_t* d_slot_base, const int64_t* d_order, const int64_t* d_sorted_keys,
                                       int64_t max_entries, float* d_slot_grad, float* d_inv, float* d_dW, int32_t chunk,
                                       float* d_scratch, int64_t scratch_bytes, void* stream)
{
    const char* where = "gp_mag_prop_rows_backward_det_drop";
    if (const int rc = mag_check(where, n_vocab, dim, n_nodes, n_rows, K, n_batch, n_samples, dropnode_rate, input_droprate,
                                 d_keep, keep_stride)) return rc;
    if (max_entries < 1 || (int64_t)n_batch * K >= (1ll << 31))
        return fail(GP_ERR_INVALID_ARG, where, "max_entries < 1 or n_batch * K >= 2^31");
    if (chunk != 0) {                                                             // DESIGN §7w's rules, as chunk_check states them
        if (!gp_gather_chunk::chunk_ok(chunk)) return fail(GP_ERR_INVALID_ARG, where, "chunk is neither 0 nor a power of two in [64, 4096]");
        const int64_t need = n_batch == 0 ? 0 : gp_gather_chunk::scratch_bytes(max_entries, chunk, dim);
        if (scratch_bytes < need) return fail(GP_ERR_INVALID_ARG, where, "the scratch is smaller than GP_GATHER_CHUNK_SCRATCH_BYTES");
        if (need > 0 && !d_scratch) return fail(GP_ERR_NULL, where, "the scratch pointer is NULL");
    }
    if (n_batch == 0) return GP_OK;
    if (!d_grad_out || !d_attr_indptr || !d_attr_indices || !d_attr_data || !d_col || !d_val || !d_slot_base || !d_order ||
        !d_sorted_keys || !d_slot_grad || !d_inv || !d_dW)
        return fail(GP_ERR_NULL, where, "a device pointer is NULL");
    if (const int rc = set_device(device, where)) return rc;
    const int n_waves = waves_for(K);
    const int nsc = std::min<int>(n_samples, (kLdsFloats - K - kMaxSamples) / K);
    const size_t lds = (size_t)(K + kMaxSamples + nsc * K) * 4;
    const MagArgs A = {n_vocab, dim, (const long long*)d_attr_indptr, d_attr_indices, d_attr_data, n_nodes, d_col, d_val, d_filled,
                       n_rows, K, d_batch_rows, n_batch, n_samples, nsc, dropnode_rate, input_droprate, training, (u64)seed,
                       d_keep, (long long)keep_stride, (const u64*)d_seed};
    hipLaunchKernelGGL(mag_slot_grad_samples_kernel, dim3(std::min<int>(n_batch, kGridCap)), dim3(n_waves * 64), lds, (hipStream_t)stream,
                       d_grad_out, A, d_slot_grad, d_inv);
    if (const int rc = launch_status("mag_slot_grad_samples_kernel")) return rc;
    const gp_mag_drop::GatherCall call = {d_slot_grad, n_vocab, dim, d_attr_indptr, d_attr_indices, d_attr_data, n_nodes, d_col, d_filled,
                                          n_rows, K, d_batch_rows, n_batch, n_samples, input_droprate,
                                          training && input_droprate > 0.0f, seed, d_seed, d_slot_base, d_order, d_sorted_keys,
                                          max_entries, d_dW, chunk, d_scratch};
    return gp_mag_drop::gather(call, stream);
}

}  // extern "C"
