// mag_prop.hip -- MAG's fused front end (grandplus_mag.h): the resident GFPush rows of a batch -> the S
// augmented embeddings `MagMLP.forward` takes, in one launch, and the gradient to the embedding table in one more.
// It replaces flatten_rows -> embedding_bag_csr(nodes) -> random_prop: no [B*K, H] intermediate, no layout rebuilt per
// call, no host read.  The op is latency-bound (about 5 MB at the MAG shape), so the mapping exposes parallelism:
//   one workgroup per batch row (grid-stride), its columns and the S weight rows staged in LDS;
//   one wave per slot, n_waves = min(16, pow2 >= K), so a wave owns at most ceil(K / 16) slots;
//   per slot the 64 lanes read 64 (id, d) pairs at once and pass them round by shuffle; the lanes sit on 64 consecutive
//   floats of W[a] (H = 64: one 256-B wave load per entry), 8 loads in flight; H > 64 loops over 64-column chunks;
//   the waves' sums meet in LDS and are added in wave order (no atomics in the forward).
// The order contract, the mask formulas and the bounds rules are stated in grandplus_mag.h.  The DropNode weight of
// (sample s, entry e) is dropnode.hpp's sample_weight, the line gp_random_prop_rows_multi calls: the same mask for the same seed.
// The forms that read the seed from device memory (mag_drop_abi.hpp) launch the same kernels, and the gather Op of
// the deterministic backward with input dropout stands here too, next to slot_seed (mag_drop_gather.hpp).
#include "mag_stage.hpp"
#include "gather_sum.hpp"
#include "gather_chunk.hpp"
#include "mag_det_layout.hpp"
#include "mag_drop_abi.hpp"
#include "mag_drop_gather.hpp"

#include <algorithm>

namespace {

constexpr u64 kSlotMul = 0xE7037ED1A0B428DBull;        // GP_MAG_SLOT_SEED's multiplier: no other derivation uses it

// GP_MAG_SLOT_SEED(seed, s, e)
__device__ __forceinline__ u64 slot_seed(u64 seed, int s, long long e)
{
    return mix64(sample_seed(seed, s) ^ ((u64)(e + 1) * kSlotMul));
}

// LDS: s_col[K] s_seen[K] s_inv[16] s_w[nsc][K] s_red[n_waves][nsc][64].  NS >= nsc accumulators per lane.
template <int NS, bool DROP>
__global__ void __launch_bounds__(kMaxWaves * 64)
mag_prop_rows_kernel(const float* __restrict__ W, MagArgs A, float* __restrict__ out, int* __restrict__ n_bad)
{
    extern __shared__ float smem[];
    const int K = A.K, H = A.H, nsc = A.nsc;
    int* s_col = reinterpret_cast<int*>(smem);
    int* s_seen = s_col + K;
    float* s_inv = smem + 2 * K;
    float* s_w = s_inv + kMaxSamples;
    float* s_red = s_w + nsc * K;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    const float scale_node = inv_keep(A.p_node);
    const float scale_in = inv_keep(A.p_in);
    const size_t out_stride = (size_t)A.B * H;
    const u64 seed = call_seed(A);
    for (int b = blockIdx.x; b < A.B; b += gridDim.x) {
        const long long row = A.batch_rows ? (long long)A.batch_rows[b] : (long long)b;
        if (row < 0 || row >= A.n_rows) {                                     // workgroup-uniform
            if (threadIdx.x == 0 && n_bad) atomicAdd(n_bad, 1);
            for (size_t i = threadIdx.x; i < (size_t)A.S * H; i += blockDim.x) {
                const size_t s = i / H, h = i - s * H;
                out[s * out_stride + (size_t)b * H + h] = 0.0f;
            }
            continue;
        }
        const int n = A.filled ? max(0, min(A.filled[row], K)) : K;             // not row_len: a negative filled[row] is 0 here
        for (int s0 = 0; s0 < A.S; s0 += nsc) {
            const int ns = min(nsc, A.S - s0);
            __syncthreads();
            stage_row(A, seed, row, n, s0, ns, scale_node, s_col, s_seen, s_w, n_bad);
            __syncthreads();
            if (threadIdx.x < ns) {
                float den = 0.0f;
                for (int k = 0; k < n; ++k) den += s_w[threadIdx.x * K + k];      // model_mag.py:85-86, sequentially in k
                s_inv[threadIdx.x] = inv_den_rows(den);
            }
            for (int hc = 0; hc < H; hc += 64) {
                const int h = hc + lane;
                const bool h_live = h < H;
                float acc[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) acc[s] = 0.0f;
                for (int k = wave; k < n; k += n_waves) {                         // wave-uniform
                    float w[NS];
                    bool any = false;
#pragma unroll
                    for (int s = 0; s < NS; ++s) { w[s] = s < ns ? s_w[s * K + k] : 0.0f; any |= w[s] != 0.0f; }
                    if (!any) continue;                                           // the bag is never read
                    const long long node = s_col[k];
                    const bool count = hc == 0 && n_bad && !s_seen[k];
                    if (hc == 0) s_seen[k] = 1;
                    const long long lo = A.indptr[node], hi = A.indptr[node + 1];
                    u64 sseed[NS];
                    float e_acc[NS];
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        e_acc[s] = 0.0f;
                        sseed[s] = DROP ? slot_seed(seed, s0 + s, row * (long long)K + k) : 0;
                    }
                    float den = 0.0f;
                    for (long long c0 = lo; c0 < hi; c0 += 64) {
                        const bool cl = c0 + lane < hi;
                        const int my_a = cl ? A.indices[c0 + lane] : -1;
                        const float my_d = cl ? A.data[c0 + lane] : 0.0f;
                        if (count && cl && (my_a < 0 || my_a >= A.V)) atomicAdd(n_bad, 1);
                        const int cnt = (int)(hi - c0 < 64 ? hi - c0 : 64);
                        for (int u0 = 0; u0 < cnt; u0 += 8) {
                            float v[8], d[8];
                            bool ok[8];
#pragma unroll
                            for (int u = 0; u < 8; ++u) {
                                const int a = __shfl(my_a, u0 + u);
                                d[u] = __shfl(my_d, u0 + u);                      // 0 past the bag's end
                                ok[u] = u0 + u < cnt && h_live && a >= 0 && a < A.V;
                                v[u] = ok[u] ? W[(size_t)a * H + h] : 0.0f;
                            }
#pragma unroll
                            for (int u = 0; u < 8; ++u) {
                                den += d[u];                                      // raw attr_data, model_mag.py:53
                                if (!ok[u]) continue;
                                if (DROP) {
                                    const u64 el = (u64)(c0 - lo + u0 + u) * (u64)H + (u64)h;
#pragma unroll
                                    for (int s = 0; s < NS; ++s)                  // F.dropout(feat_embeds), model_mag.py:50
                                        if (w[s] != 0.0f) e_acc[s] += (v[u] * keep_scale(sseed[s], el, A.p_in, scale_in)) * d[u];
                                } else {
                                    e_acc[0] += v[u] * d[u];                      // model_mag.py:52
                                }
                            }
                        }
                    }
                    const float inv_den = inv_den_bag(den);                  // model_mag.py:54
#pragma unroll
                    for (int s = 0; s < NS; ++s) acc[s] += w[s] * (e_acc[DROP ? s : 0] * inv_den);   // model_mag.py:83-84
                }
#pragma unroll
                for (int s = 0; s < NS; ++s)
                    if (s < ns) s_red[(wave * nsc + s) * 64 + lane] = acc[s];
                __syncthreads();
                for (int i = threadIdx.x; i < ns * 64; i += blockDim.x) {
                    const int s = i >> 6, l = i & 63;
                    float sum = 0.0f;
                    for (int wv = 0; wv < n_waves; ++wv) sum += s_red[(wv * nsc + s) * 64 + l];   // waves in order
                    if (hc + l < H) out[(size_t)(s0 + s) * out_stride + (size_t)b * H + hc + l] = sum * s_inv[s];
                }
                __syncthreads();
            }
        }
    }
}

// Backward.  LDS: s_col[K] s_inv[16] s_w[nsc][K].  One atomic per (entry, h) and sample chunk; a chunk is up to 16 samples,
// 8 with input dropout (every sample then keeps its own scaled gradient and hash seed in registers).
template <bool DROP>
__global__ void __launch_bounds__(kMaxWaves * 64)
mag_prop_rows_backward_kernel(const float* __restrict__ grad_out, MagArgs A, float* __restrict__ dW)
{
    extern __shared__ float smem[];
    constexpr int MS = DROP ? kMaxSamples / 2 : kMaxSamples;
    const int K = A.K, H = A.H, nsc = A.nsc;
    int* s_col = reinterpret_cast<int*>(smem);
    float* s_inv = smem + K;
    float* s_w = s_inv + kMaxSamples;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    const float scale_node = inv_keep(A.p_node);
    const float scale_in = inv_keep(A.p_in);
    const size_t g_stride = (size_t)A.B * H;
    const u64 seed = call_seed(A);
    for (int b = blockIdx.x; b < A.B; b += gridDim.x) {
        const long long row = A.batch_rows ? (long long)A.batch_rows[b] : (long long)b;
        if (row < 0 || row >= A.n_rows) continue;                                 // workgroup-uniform
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
            }
            __syncthreads();
            for (int hc = 0; hc < H; hc += 64) {
                const int h = hc + lane;
                const bool h_live = h < H;
                float gs[MS];
#pragma unroll
                for (int s = 0; s < MS; ++s)
                    gs[s] = s < ns && h_live ? grad_out[(size_t)(s0 + s) * g_stride + (size_t)b * H + h] * s_inv[s] : 0.0f;
                for (int k = wave; k < n; k += n_waves) {                         // wave-uniform
                    bool any = false;
                    for (int s = 0; s < ns; ++s) any |= s_w[s * K + k] != 0.0f;
                    if (!any) continue;
                    const long long node = s_col[k];
                    const long long lo = A.indptr[node], hi = A.indptr[node + 1];
                    float den = 0.0f;
                    for (long long c0 = lo; c0 < hi; c0 += 64) {                  // sequentially in t, as the forward
                        const float my_d = c0 + lane < hi ? A.data[c0 + lane] : 0.0f;
                        const int cnt = (int)(hi - c0 < 64 ? hi - c0 : 64);
                        for (int u = 0; u < cnt; ++u) den += __shfl(my_d, u);
                    }
                    const float inv_den = inv_den_bag(den);
                    float cs[MS], c = 0.0f;
                    u64 sseed[MS];
#pragma unroll
                    for (int s = 0; s < MS; ++s) {
                        const float ws = s < ns ? s_w[s * K + k] : 0.0f;
                        const float x = gs[s] * ws;
                        if (s < ns) c += x;                                       // s ascending, from 0.0f
                        cs[s] = DROP && ws != 0.0f ? x * inv_den : 0.0f;
                        sseed[s] = DROP && ws != 0.0f ? slot_seed(seed, s0 + s, row * (long long)K + k) : 0;
                    }
                    const float cd = c * inv_den;
                    for (long long c0 = lo; c0 < hi; c0 += 64) {
                        const bool cl = c0 + lane < hi;
                        const int my_a = cl ? A.indices[c0 + lane] : -1;
                        const float my_d = cl ? A.data[c0 + lane] : 0.0f;
                        const int cnt = (int)(hi - c0 < 64 ? hi - c0 : 64);
                        for (int u = 0; u < cnt; ++u) {
                            const int a = __shfl(my_a, u);
                            const float d = __shfl(my_d, u);
                            if (a < 0 || a >= A.V) continue;                      // wave-uniform
                            float x;
                            if (DROP) {
                                const u64 el = (u64)(c0 - lo + u) * (u64)H + (u64)h;
                                x = 0.0f;
#pragma unroll
                                for (int s = 0; s < MS; ++s)
                                    if (cs[s] != 0.0f) x += (cs[s] * d) * keep_scale(sseed[s], el, A.p_in, scale_in);
                            } else {
                                x = cd * d;
                            }
                            if (h_live && x != 0.0f) atomicAdd(dW + (size_t)a * H + h, x);
                        }
                    }
                }
            }
        }
    }
}

// Accumulators per lane of the forward: S rounded up to a power of two, at most 8; more samples take several chunks.
// With input dropout every sample also keeps its own bag sum and hash seed, and a chunk is 2 samples: 4 would spill.
int forward_ns(int S, bool drop) { return S <= 1 ? 1 : S <= 2 || drop ? 2 : S <= 4 ? 4 : 8; }

// ---- what one sorted position contributes to the deterministic backward with input dropout (the Op of
// gather_sum_kernel and gather_chunk.hpp, as mag_det.hip's MagOp).  The order contract is mag_drop_abi.hpp's: per entry the
// samples' U[s, e, :] * d, each under its own mask, s ascending from 0.0f; then the destination's sum in entry order.
// A sample whose U is 0 adds a zero to a sum that began at +0.0f: passing it over gives the same bits and saves its hash.
struct MagDropOp {
    const float* U; int H, S; SlotArgs A; const float* data; const long long* slot_base; long long n_slots, max_entries;
    int drop; float p_in; u64 seed; const u64* d_seed;

    struct Entry { long long e, rslot, t; float d; int live; u64 seed; };

    __device__ __forceinline__ Entry load(const long long* __restrict__ order, long long i, bool want, long long key) const
    {
        Entry E;
        E.e = 0; E.rslot = 0; E.t = 0; E.d = 0.0f; E.live = 0;
        E.seed = d_seed ? *d_seed : seed;                             // wave-uniform: once per window of sorted positions
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
        const long long b = e / A.K;
        const long long row = A.batch_rows ? (long long)A.batch_rows[b] : b;   // in [0, n_rows): slot_node said so
        E.e = e; E.rslot = row * (long long)A.K + (e - b * A.K); E.t = t; E.d = data[lo + t]; E.live = 1;
        return E;
    }

    __device__ __forceinline__ void add(const Entry& E, int u, int f, float (&acc)[kCols]) const
    {
        if (!__shfl(E.live, u)) return;                              // wave-uniform
        const long long e = __shfl(E.e, u), rslot = __shfl(E.rslot, u), t = __shfl(E.t, u);
        const float d = __shfl(E.d, u);
        const float scale_in = inv_keep(p_in);
        float x[kCols];
#pragma unroll
        for (int c = 0; c < kCols; ++c) x[c] = 0.0f;
        for (int s = 0; s < S; ++s) {                                 // s ascending, from 0.0f
            const float* up = U + ((size_t)s * (size_t)n_slots + (size_t)e) * H;
            const u64 sseed = drop ? slot_seed(E.seed, s, rslot) : 0;
#pragma unroll
            for (int c = 0; c < kCols; ++c) {
                const int h = f + 64 * c;
                if (h >= H) continue;
                const float us = up[h];
                if (us == 0.0f) continue;
                const float xd = us * d;
                x[c] += drop ? xd * keep_scale(sseed, (u64)t * (u64)H + (u64)h, p_in, scale_in) : xd;
            }
        }
#pragma unroll
        for (int c = 0; c < kCols; ++c)
            if (f + 64 * c < H) acc[c] += x[c];
    }
};

// The two forms of the forward share everything but where the seed stands: `seed` itself, or *d_seed on the device.
int mag_forward(const char* where, int device, const float* d_weight, int64_t n_vocab, int32_t dim, const int64_t* d_attr_indptr,
                const int32_t* d_attr_indices, const float* d_attr_data, int64_t n_nodes, const int32_t* d_col, const double* d_val,
                const int32_t* d_filled, int64_t n_rows, int32_t K, const int32_t* d_batch_rows, int32_t n_batch, int32_t n_samples,
                float dropnode_rate, float input_droprate, int training, uint64_t seed, const uint64_t* d_seed, bool device_seed,
                const uint8_t* d_keep, int64_t keep_stride, float* d_out, int32_t* d_n_bad, void* stream)
{
    if (const int rc = mag_check(where, n_vocab, dim, n_nodes, n_rows, K, n_batch, n_samples, dropnode_rate, input_droprate,
                                 d_keep, keep_stride)) return rc;
    if (n_batch == 0) return GP_OK;
    if (!d_weight || !d_attr_indptr || !d_attr_indices || !d_attr_data || !d_col || !d_val || !d_out || (device_seed && !d_seed))
        return fail(GP_ERR_NULL, where, "a device pointer is NULL");
    if (const int rc = set_device(device, where)) return rc;
    const bool drop = training && input_droprate > 0.0f;
    const int n_waves = waves_for(K), ns = forward_ns(n_samples, drop);
    const int fit = (kLdsFloats - 2 * K - kMaxSamples) / (K + n_waves * 64);
    const int nsc = std::min(std::min(ns, fit), (int)n_samples);
    const size_t lds = (size_t)(2 * K + kMaxSamples + nsc * K + n_waves * nsc * 64) * 4;
    const MagArgs A = {n_vocab, dim, (const long long*)d_attr_indptr, d_attr_indices, d_attr_data, n_nodes, d_col, d_val, d_filled,
                       n_rows, K, d_batch_rows, n_batch, n_samples, nsc, dropnode_rate, input_droprate, training, (u64)seed,
                       d_keep, (long long)keep_stride, (const u64*)d_seed};
    const dim3 grid(std::min<int>(n_batch, kGridCap)), block(n_waves * 64);
    hipStream_t s = (hipStream_t)stream;
#define GP_MAG_FWD(N, D) hipLaunchKernelGGL((mag_prop_rows_kernel<N, D>), grid, block, lds, s, d_weight, A, d_out, d_n_bad)
    if (drop) { if (ns == 1) GP_MAG_FWD(1, true); else GP_MAG_FWD(2, true); }
    else      { if (ns == 1) GP_MAG_FWD(1, false); else if (ns == 2) GP_MAG_FWD(2, false); else if (ns == 4) GP_MAG_FWD(4, false); else GP_MAG_FWD(8, false); }
#undef GP_MAG_FWD
    return launch_status("mag_prop_rows_kernel");
}

int mag_backward(const char* where, int device, const float* d_grad_out, int64_t n_vocab, int32_t dim, const int64_t* d_attr_indptr,
                 const int32_t* d_attr_indices, const float* d_attr_data, int64_t n_nodes, const int32_t* d_col, const double* d_val,
                 const int32_t* d_filled, int64_t n_rows, int32_t K, const int32_t* d_batch_rows, int32_t n_batch, int32_t n_samples,
                 float dropnode_rate, float input_droprate, int training, uint64_t seed, const uint64_t* d_seed, bool device_seed,
                 const uint8_t* d_keep, int64_t keep_stride, float* d_dW, void* stream)
{
    if (const int rc = mag_check(where, n_vocab, dim, n_nodes, n_rows, K, n_batch, n_samples, dropnode_rate, input_droprate,
                                 d_keep, keep_stride)) return rc;
    if (n_batch == 0) return GP_OK;
    if (!d_grad_out || !d_attr_indptr || !d_attr_indices || !d_attr_data || !d_col || !d_val || !d_dW || (device_seed && !d_seed))
        return fail(GP_ERR_NULL, where, "a device pointer is NULL");
    if (const int rc = set_device(device, where)) return rc;
    const int n_waves = waves_for(K);
    const bool drop = training && input_droprate > 0.0f;
    const int nsc = std::min(std::min<int>(n_samples, drop ? kMaxSamples / 2 : kMaxSamples), (kLdsFloats - K - kMaxSamples) / K);
    const size_t lds = (size_t)(K + kMaxSamples + nsc * K) * 4;
    const MagArgs A = {n_vocab, dim, (const long long*)d_attr_indptr, d_attr_indices, d_attr_data, n_nodes, d_col, d_val, d_filled,
                       n_rows, K, d_batch_rows, n_batch, n_samples, nsc, dropnode_rate, input_droprate, training, (u64)seed,
                       d_keep, (long long)keep_stride, (const u64*)d_seed};
    const dim3 grid(std::min<int>(n_batch, kGridCap)), block(n_waves * 64);
    if (drop)
        hipLaunchKernelGGL(mag_prop_rows_backward_kernel<true>, grid, block, lds, (hipStream_t)stream, d_grad_out, A, d_dW);
    else
        hipLaunchKernelGGL(mag_prop_rows_backward_kernel<false>, grid, block, lds, (hipStream_t)stream, d_grad_out, A, d_dW);
    return launch_status("mag_prop_rows_backward_kernel");
}

}  // namespace

// mag_drop_gather.hpp: the gather of gp_mag_prop_rows_backward_det_drop, whose checks, U and inv are mag_drop.hip's.
int gp_mag_drop::gather(const GatherCall& c, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    const MagDropOp op = {c.U, c.dim, c.n_samples,
                          {(const long long*)c.attr_indptr, c.attr_indices, c.n_nodes, c.n_vocab, c.col, c.filled, c.n_rows, c.K,
                           c.batch_rows},
                          c.attr_data, (const long long*)c.slot_base, (long long)c.n_batch * c.K, (long long)c.max_entries,
                          c.drop, c.input_droprate, (u64)c.seed, (const u64*)c.d_seed};
    if (c.chunk == 0) {
        hipLaunchKernelGGL(gather_sum_kernel<MagDropOp>, dim3(gather_grid(c.max_entries)), dim3(kGather), 0, s, op,
                           (const long long*)c.order, (const long long*)c.sorted_keys, (long long)c.max_entries, (long long)c.n_vocab,
                           c.dim, c.dW);
        return launch_status("gather_sum_kernel<MagDropOp>");
    }
    return gather_chunked(op, "gather_chunk_kernel<MagDropOp>", c.order, c.sorted_keys, c.max_entries, c.n_vocab, c.dim, c.chunk, c.dW,
                          c.scratch, s);
}

extern "C" {

int gp_mag_prop_rows(int device, const float* d_weight, int64_t n_vocab, int32_t dim, const int64_t* d_attr_indptr,
                     const int32_t* d_attr_indices, const float* d_attr_data, int64_t n_nodes, const int32_t* d_col,
                     const double* d_val, const int32_t* d_filled, int64_t n_rows, int32_t K,
                     const int32_t* d_batch_rows, int32_t n_batch, int32_t n_samples, float dropnode_rate,
                     float input_droprate, int training, uint64_t seed, const uint8_t* d_keep, int64_t keep_stride,
                     float* d_out, int32_t* d_n_bad, void* stream)
{
    return mag_forward("gp_mag_prop_rows", device, d_weight, n_vocab, dim, d_attr_indptr, d_attr_indices, d_attr_data, n_nodes, d_col,
                       d_val, d_filled, n_rows, K, d_batch_rows, n_batch, n_samples, dropnode_rate, input_droprate, training, seed,
                       nullptr, false, d_keep, keep_stride, d_out, d_n_bad, stream);
}

int gp_mag_prop_rows_dseed(int device, const float* d_weight, int64_t n_vocab, int32_t dim, const int64_t* d_attr_indptr,
                           const int32_t* d_attr_indices, const float* d_attr_data, int64_t n_nodes, const int32_t* d_col,
                           const double* d_val, const int32_t* d_filled, int64_t n_rows, int32_t K,
                           const int32_t* d_batch_rows, int32_t n_batch, int32_t n_samples, float dropnode_rate,
                           float input_droprate, int training, const uint64_t* d_seed, const uint8_t* d_keep,
                           int64_t keep_stride, float* d_out, int32_t* d_n_bad, void* stream)
{
    return mag_forward("gp_mag_prop_rows_dseed", device, d_weight, n_vocab, dim, d_attr_indptr, d_attr_indices, d_attr_data, n_nodes,
                       d_col, d_val, d_filled, n_rows, K, d_batch_rows, n_batch, n_samples, dropnode_rate, input_droprate, training, 0,
                       d_seed, true, d_keep, keep_stride, d_out, d_n_bad, stream);
}

int gp_mag_prop_rows_backward(int device, const float* d_grad_out, int64_t n_vocab, int32_t dim,
                              const int64_t* d_attr_indptr, const int32_t* d_attr_indices, const float* d_attr_data,
                              int64_t n_nodes, const int32_t* d_col, const double* d_val, const int32_t* d_filled,
                              int64_t n_rows, int32_t K, const int32_t* d_batch_rows, int32_t n_batch,
                              int32_t n_samples, float dropnode_rate, float input_droprate, int training,
                              uint64_t seed, const uint8_t* d_keep, int64_t keep_stride, float* d_dW, void* stream)
{
    return mag_backward("gp_mag_prop_rows_backward", device, d_grad_out, n_vocab, dim, d_attr_indptr, d_attr_indices, d_attr_data,
                        n_nodes, d_col, d_val, d_filled, n_rows, K, d_batch_rows, n_batch, n_samples, dropnode_rate, input_droprate,
                        training, seed, nullptr, false, d_keep, keep_stride, d_dW, stream);
}

int gp_mag_prop_rows_backward_dseed(int device, const float* d_grad_out, int64_t n_vocab, int32_t dim,
                                    const int64_t* d_attr_indptr, const int32_t* d_attr_indices, const float* d_attr_data,
                                    int64_t n_nodes, const int32_t* d_col, const double* d_val, const int32_t* d_filled,
                                    int64_t n_rows, int32_t K, const int32_t* d_batch_rows, int32_t n_batch,
                                    int32_t n_samples, float dropnode_rate, float input_droprate, int training,
                                    const uint64_t* d_seed, const uint8_t* d_keep, int64_t keep_stride, float* d_dW,
                                    void* stream)
{
    return mag_backward("gp_mag_prop_rows_backward_dseed", device, d_grad_out, n_vocab, dim, d_attr_indptr, d_attr_indices,
                        d_attr_data, n_nodes, d_col, d_val, d_filled, n_rows, K, d_batch_rows, n_batch, n_samples, dropnode_rate,
                        input_droprate, training, 0, d_seed, true, d_keep, keep_stride, d_dW, stream);
}

}  // extern "C"
