// augment.hip -- SURVEY.md 8(f) next-1: GRAND+'s feature augmentation ("random propagation"),
// reference Grand_Plus.random_prop (model.py:80-87; model_mag.py:80-86):
//
//     s    = dropout(mat_scores, p)                          (model.py:82)
//     num  = scatter_sum(feats * s[:, None], mat_idx)        (model.py:83-84)   torch_scatter, fp32
//     den  = scatter_sum(s[:, None], mat_idx)                (model.py:85-86)
//     out  = num / (den + 1e-12)                             (model.py:87)
//
// One fused gfx950 kernel: a workgroup owns one output row, stages that row's (column, weight)
// pairs in LDS, applies DropNode there, and every lane accumulates 4 feature columns over the
// row's neighbours with 16-byte loads of whole feature rows (the op is an HBM gather:
// filled*F*4 B per output row; a [1xK]x[KxF] product per row has no reuse for MFMA to exploit).
// Dropped neighbours are never read.  Two entry points:
//   gp_random_prop_rows : reads the [S x K] rows GFPush left in HBM (col i32, val f64, filled)
//                         and the node-feature matrix X[N x F] -- no gather on the host, no
//                         per-step upload (the caller side of model.py:310-316).
//   gp_random_prop_coo  : the reference's own argument shape (gathered feats [M x F],
//                         scores [M], sorted segment ids [M]).
// The DropNode weight, the row length, the denominators and the bag are dropnode.hpp's, shared with scatter_det.hip and mag_prop.hip.
#include "dropnode.hpp"

#include <algorithm>

namespace {

constexpr int kBlock = 256;

// Accumulates out[b, f0:f1] = sum_k w_k * X[c_k, f0:f1] / (sum_k w_k + 1e-12) for the staged (c_k, w_k).
// VEC floats per lane per access (4 when F % 4 == 0, 2 when F % 2 == 0, else 1); blockIdx.y selects
// the slab of kBlock*VEC feature columns, so small batches still spread over many workgroups; 8
// feature rows are in flight per lane.
template <int VEC>
__device__ __forceinline__ void weighted_rows_vec(const float* __restrict__ X, int F, const int* s_col,
                                                  const float* s_w, int n, float* __restrict__ out_row)
{
    typedef typename VecT<VEC>::type V;
    float den = 0.0f;
    for (int k = 0; k < n; ++k) den += s_w[k];                                    // model.py:85-86
    const float inv = inv_den_rows(den);                                      // model.py:87
    for (int f = (blockIdx.y * kBlock + threadIdx.x) * VEC; f < F; f += gridDim.y * kBlock * VEC) {
        float acc[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] = 0.0f;
        int k = 0;
        for (; k + 8 <= n; k += 8) {
            V v[8]; float w[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                w[u] = s_w[k + u];
                const int c = w[u] != 0.0f ? s_col[k + u] : s_col[k];            // dropped neighbours re-read a line already in flight
                v[u] = *reinterpret_cast<const V*>(X + (size_t)c * F + f);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float* pv = reinterpret_cast<const float*>(&v[u]);
#pragma unroll
                for (int i = 0; i < VEC; ++i) acc[i] += w[u] * pv[i];             // model.py:83-84
            }
        }
        for (; k < n; ++k) {
            const float w = s_w[k];
            if (w == 0.0f) continue;
            const V v = *reinterpret_cast<const V*>(X + (size_t)s_col[k] * F + f);
            const float* pv = reinterpret_cast<const float*>(&v);
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] += w * pv[i];
        }
        V o; float* po = reinterpret_cast<float*>(&o);
#pragma unroll
        for (int i = 0; i < VEC; ++i) po[i] = acc[i] * inv;
        *reinterpret_cast<V*>(out_row + f) = o;
    }
}

__device__ __forceinline__ void weighted_rows(const float* __restrict__ X, int F, const int* s_col,
                                              const float* s_w, int n, float* __restrict__ out_row)
{
    if ((F & 3) == 0)      weighted_rows_vec<4>(X, F, s_col, s_w, n, out_row);
    else if ((F & 1) == 0) weighted_rows_vec<2>(X, F, s_col, s_w, n, out_row);
    else                   weighted_rows_vec<1>(X, F, s_col, s_w, n, out_row);
}

__global__ void __launch_bounds__(kBlock)
random_prop_rows_kernel(const float* __restrict__ X, int F, const int* __restrict__ col,
                        const double* __restrict__ val, const int* __restrict__ filled, int K,
                        const int* __restrict__ batch_rows, int n_batch, float p, int training, u64 seed,
                        const unsigned char* __restrict__ keep, float* __restrict__ out)
{
    __shared__ int s_col[kStage];
    __shared__ float s_w[kStage];
    const float scale = inv_keep(p);
    for (int b = blockIdx.x; b < n_batch; b += gridDim.x) {
        const long long row = batch_rows ? batch_rows[b] : b;
        const int n = row_len(filled, row, K);
        __syncthreads();
        for (int k = threadIdx.x; k < n; k += kBlock) {
            const long long e = row * (long long)K + k;
            float w = (float)val[e];                 // torch.tensor(mat_scores, dtype=torch.float32), model.py:314
            if (training) w *= keep ? (keep[e] ? scale : 0.0f) : keep_scale(seed, (u64)e, p, scale);   // model.py:82
            s_col[k] = col[e];
            s_w[k] = w;
        }
        __syncthreads();
        weighted_rows(X, F, s_col, s_w, n, out + (size_t)b * F);
    }
}

__global__ void __launch_bounds__(kBlock)
random_prop_coo_kernel(const float* __restrict__ feats, int F, const float* __restrict__ scores,
                       const long long* __restrict__ idx, long long n_entries, long long n_out,
                       float p, int training, u64 seed, const unsigned char* __restrict__ keep,
                       float* __restrict__ out)
{
    __shared__ int s_col[kStage];
    __shared__ float s_w[kStage];
    __shared__ long long s_lo, s_hi;
    const float scale = inv_keep(p);
    for (long long b = blockIdx.x; b < n_out; b += gridDim.x) {
        __syncthreads();
        if (threadIdx.x < 2) {                        // segment of output row b in the sorted id array
            const long long key = b + threadIdx.x;    // lower_bound(idx, b) and lower_bound(idx, b+1)
            long long lo = 0, hi = n_entries;
            while (lo < hi) { const long long mid = (lo + hi) >> 1; if (idx[mid] < key) lo = mid + 1; else hi = mid; }
            if (threadIdx.x == 0) s_lo = lo; else s_hi = lo;
        }
        __syncthreads();
        const long long lo = s_lo, hi = s_hi;
        float* out_row = out + (size_t)b * F;
        if (hi - lo <= kStage) {
            const int n = (int)(hi - lo);
            for (int k = threadIdx.x; k < n; k += kBlock) {
                const long long e = lo + k;
                float w = scores[e];
                if (training) w *= keep ? (keep[e] ? scale : 0.0f) : keep_scale(seed, (u64)e, p, scale);
                s_col[k] = (int)e;                    // feats is already gathered: entry e uses feats[e, :]
                s_w[k] = w;
            }
            __syncthreads();
            weighted_rows(feats, F, s_col, s_w, n, out_row);
        } else {
            // segment longer than the LDS stage (never for GRAND+ rows, K <= 1024): plain loop
            float den = 0.0f;
            for (long long e = lo; e < hi; ++e) {
                float w = scores[e];
                if (training) w *= keep ? (keep[e] ? scale : 0.0f) : keep_scale(seed, (u64)e, p, scale);
                den += w;
            }
            const float inv = inv_den_rows(den);
            for (int f = blockIdx.y * kBlock + threadIdx.x; f < F; f += gridDim.y * kBlock) {
                float acc = 0.0f;
                for (long long e = lo; e < hi; ++e) {
                    float w = scores[e];
                    if (training) w *= keep ? (keep[e] ? scale : 0.0f) : keep_scale(seed, (u64)e, p, scale);
                    if (w != 0.0f) acc += w * feats[(size_t)e * F + f];
                }
                out_row[f] = acc * inv;
            }
        }
    }
}

// ---- Backward of random_prop.  Scores are constants (the reference builds them from numpy,
// model_mag.py:342-343), so only the feature operand gets a gradient:
//     d out[b,:] / d feats[e,:] = w'_e / (den_b + 1e-12),   b = idx[e]
// w'_e and den_b are recomputed exactly as the forward computes them (same staging, same keep decision from
// (seed, e) or d_keep, same sequential fp32 sum), so the backward applies the forward's mask without storing it.

// COO form: a pure gather and stream.  Workgroup per output row b; every entry of the row's segment is
// written (dropped entries get exact zeros), and the workgroup of the last output row also writes the entries the
// caller's n_out cuts off (zero_cut_rows), so every row of grad_feats is written.  No atomics.

// Entries [first, n_entries) have idx >= n_out: the forward left them out, so their gradient is exactly 0.  `first` is the
// last output row's segment end, which that row's workgroup has already searched: no trip when n_out covers every entry.
__device__ __forceinline__ void zero_cut_rows(float* __restrict__ grad_feats, int F, long long first, long long n_entries)
{
    const size_t end = (size_t)n_entries * F;
    for (size_t t = (size_t)first * F + threadIdx.x; t < end; t += kBlock) grad_feats[t] = 0.0f;
}

template <int VEC>
__device__ __forceinline__ void scaled_rows_vec(const float* __restrict__ g_row, int F, const float* s_w, int n,
                                                float inv, float* __restrict__ out_rows)
{
    typedef typename VecT<VEC>::type V;
    const int FV = F / VEC;
    for (int t = threadIdx.x; t < n * FV; t += kBlock) {
        const int k = t / FV, f = (t - k * FV) * VEC;
        const V g = *reinterpret_cast<const V*>(g_row + f);
        const float* pg = reinterpret_cast<const float*>(&g);
        const float w = s_w[k];
        V o; float* po = reinterpret_cast<float*>(&o);
#pragma unroll
        for (int i = 0; i < VEC; ++i) po[i] = (pg[i] * inv) * w;
        *reinterpret_cast<V*>(out_rows + (size_t)k * F + f) = o;
    }
}

__global__ void __launch_bounds__(kBlock)
random_prop_coo_backward_kernel(const float* __restrict__ grad_out, int F, const float* __restrict__ scores,
                                const long long* __restrict__ idx, long long n_entries, long long n_out,
                                float p, int training, u64 seed, const unsigned char* __restrict__ keep,
                                float* __restrict__ grad_feats)
{
    __shared__ float s_w[kStage];
    __shared__ long long s_lo, s_hi;
    const float scale = inv_keep(p);
    for (long long b = blockIdx.x; b < n_out; b += gridDim.x) {
        __syncthreads();
        if (threadIdx.x < 2) {                        // the forward's segment search
            const long long key = b + threadIdx.x;
            long long lo = 0, hi = n_entries;
            while (lo < hi) { const long long mid = (lo + hi) >> 1; if (idx[mid] < key) lo = mid + 1; else hi = mid; }
            if (threadIdx.x == 0) s_lo = lo; else s_hi = lo;
        }
        __syncthreads();
        const long long lo = s_lo, hi = s_hi;
        const float* g_row = grad_out + (size_t)b * F;
        if (hi - lo <= kStage) {
            const int n = (int)(hi - lo);
            for (int k = threadIdx.x; k < n; k += kBlock) {
                const long long e = lo + k;
                float w = scores[e];
                if (training) w *= keep ? (keep[e] ? scale : 0.0f) : keep_scale(seed, (u64)e, p, scale);
                s_w[k] = w;
            }
            __syncthreads();
            float den = 0.0f;
            for (int k = 0; k < n; ++k) den += s_w[k];                      // the forward's order
            const float inv = inv_den_rows(den);
            float* rows = grad_feats + (size_t)lo * F;
            if ((F & 3) == 0)      scaled_rows_vec<4>(g_row, F, s_w, n, inv, rows);
            else if ((F & 1) == 0) scaled_rows_vec<2>(g_row, F, s_w, n, inv, rows);
            else                   scaled_rows_vec<1>(g_row, F, s_w, n, inv, rows);
        } else {
            float den = 0.0f;
            for (long long e = lo; e < hi; ++e) {
                float w = scores[e];
                if (training) w *= keep ? (keep[e] ? scale : 0.0f) : keep_scale(seed, (u64)e, p, scale);
                den += w;
            }
            const float inv = inv_den_rows(den);
            for (long long e = lo; e < hi; ++e) {
                float w = scores[e];
                if (training) w *= keep ? (keep[e] ? scale : 0.0f) : keep_scale(seed, (u64)e, p, scale);
                for (int f = threadIdx.x; f < F; f += kBlock) grad_feats[(size_t)e * F + f] = (g_row[f] * inv) * w;
            }
        }
        if (b == n_out - 1) zero_cut_rows(grad_feats, F, hi, n_entries);
    }
}

// Fused form: grad_X[col[r,k], :] += w'_{r,k} / (den_b + 1e-12) * grad_out[b, :] into a caller-zeroed grad_X.
// A node can occur in many rows (and twice in one row), so fp32 global atomics.  Each wave takes one staged
// entry at a time and its 64 lanes add 64 consecutive floats of that entry's destination row: one 256-B
// contiguous global_atomic_add_f32 wave-instruction per 64 columns (the full-rate shape).
__global__ void __launch_bounds__(kBlock)
random_prop_rows_backward_kernel(const float* __restrict__ grad_out, int F, const int* __restrict__ col,
                                 const double* __restrict__ val, const int* __restrict__ filled, int K,
                                 const int* __restrict__ batch_rows, int n_batch, long long n_nodes,
                                 float p, int training, u64 seed, const unsigned char* __restrict__ keep,
                                 float* __restrict__ grad_x)
{
    __shared__ int s_col[kStage];
    __shared__ float s_w[kStage];
    const float scale = inv_keep(p);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int b = blockIdx.x; b < n_batch; b += gridDim.x) {
        const long long row = batch_rows ? batch_rows[b] : b;
        const int n = row_len(filled, row, K);
        __syncthreads();
        for (int k = threadIdx.x; k < n; k += kBlock) {                  // the forward's staging
            const long long e = row * (long long)K + k;
            float w = (float)val[e];
            if (training) w *= keep ? (keep[e] ? scale : 0.0f) : keep_scale(seed, (u64)e, p, scale);
            s_col[k] = col[e];
            s_w[k] = w;
        }
        __syncthreads();
        float den = 0.0f;
        for (int k = 0; k < n; ++k) den += s_w[k];
        const float inv = inv_den_rows(den);
        const float* g_row = grad_out + (size_t)b * F;
        for (int k = wave; k < n; k += kBlock / 64) {
            const float w = s_w[k];
            const int c = s_col[k];
            if (w == 0.0f || c < 0 || c >= n_nodes) continue;           // wave-uniform; a dropped entry adds nothing
            float* dst = grad_x + (size_t)c * F;
            for (int f = lane; f < F; f += 64) atomicAdd(dst + f, (g_row[f] * inv) * w);
        }
    }
}

// ---- Embedding-bag: dropnode.hpp states the bag and holds BagLayout, bag_of and attr_id.

// Forward: propagate.hip's mapping -- a group of G = 2^log2g lanes owns one output row (G*VEC >= H when H
// allows), fp32 sums.  The group's lanes first read G entries' (id, weight) at once, one per lane, and pass
// them round with shuffles (a bag costs one dependent read round per G entries, not one per 8); then 8
// gathered table rows are in flight per lane.  A dropped element is still loaded (its row is being read
// anyway); an out-of-range id is not.
template <int VEC>
__global__ void __launch_bounds__(kBlock)
embedding_bag_kernel(const float* __restrict__ W, long long V, int H, BagLayout L, float p, int training, u64 seed,
                     const unsigned char* __restrict__ keep, float* __restrict__ out, int* __restrict__ n_bad, int log2g)
{
    typedef typename VecT<VEC>::type Vt;
    const float scale = inv_keep(p);
    const int lane = threadIdx.x & 63;
    const int G = 1 << log2g, gl = lane & (G - 1), grp = lane >> log2g, rows_per_wave = 64 >> log2g;
    const long long wave = ((long long)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const long long n_waves = ((long long)gridDim.x * kBlock) >> 6;
    const long long n_iter = (L.n_rows + n_waves * rows_per_wave - 1) / (n_waves * rows_per_wave);
    for (long long it = 0; it < n_iter; ++it) {                     // every lane runs every trip: shuffles need the whole wave
        const long long m = (it * n_waves + wave) * rows_per_wave + grp;
        const bool row_live = m < L.n_rows;
        long long s0 = 0, s1 = 0, jb = 0;
        if (row_live && !bag_of(L, m, s0, s1, jb) && gl == 0 && n_bad) atomicAdd(n_bad, 1);
        long long len = s1 - s0, max_len = len;                     // the wave loops over its longest bag
        for (int o = G; o < 64; o <<= 1) { const long long t = __shfl_xor(max_len, o); max_len = t > max_len ? t : max_len; }
        const int n_f = (H + G * VEC - 1) / (G * VEC);
        for (int fi = 0; fi < n_f; ++fi) {
            const int f = (fi * G + gl) * VEC;
            const bool f_live = f < H;
            float acc[VEC], den = 0.0f;
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = 0.0f;
            for (long long c0 = 0; c0 < max_len; c0 += G) {
                const bool cl = c0 + gl < len;                      // this lane reads entry c0 + gl of its group's bag
                const long long my_a = cl ? attr_id(L, s0 + c0 + gl) : -1;
                const float my_d = cl ? L.data[s0 + c0 + gl] : 0.0f;
                if (cl && (my_a < 0 || my_a >= V) && fi == 0 && n_bad) atomicAdd(n_bad, 1);
                for (int u0 = 0; u0 < G && c0 + u0 < max_len; u0 += 8) {
                    Vt v[8]; float d[8]; bool ok[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int src = (grp << log2g) + ((u0 + u) & (G - 1));
                        const long long a = __shfl(my_a, src);
                        d[u] = __shfl(my_d, src);
                        const bool live = u0 + u < G && c0 + u0 + u < len;
                        ok[u] = live && f_live && a >= 0 && a < V;
                        if (!live) d[u] = 0.0f;
                        if (ok[u]) v[u] = *reinterpret_cast<const Vt*>(W + (size_t)a * H + f);
                        else v[u] = Vt();
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        den += d[u];                                            // node_s_sum, model_mag.py:53 (raw attr_data)
                        if (!ok[u]) continue;
                        const float* pv = reinterpret_cast<const float*>(&v[u]);
                        const u64 j = (u64)(jb + c0 + u0 + u);
#pragma unroll
                        for (int i = 0; i < VEC; ++i) {
                            float x = pv[i];
                            if (training) {                                     // F.dropout(feat_embeds), model_mag.py:50
                                const u64 el = j * (u64)H + (u64)(f + i);
                                x *= keep ? (keep[el] ? scale : 0.0f) : keep_scale(seed, el, p, scale);
                            }
                            acc[i] += x * d[u];                                 // model_mag.py:52
                        }
                    }
                }
            }
            if (row_live && f_live) {
                Vt o; float* po = reinterpret_cast<float*>(&o);
#pragma unroll
                for (int i = 0; i < VEC; ++i) po[i] = acc[i] / (den + 1e-10f); // model_mag.py:54 (a quotient; inv_den_bag's epsilon)
                *reinterpret_cast<Vt*>(out + (size_t)m * H + f) = o;
            }
        }
    }
}

// Backward into a dense, zeroed dW [V x H] (nn.Embedding(sparse=False)):
//     dW[a_j, :] += keep_{j,:} s d_j / (den_m + 1e-10) * grad_out[m, :]
// A wave owns an output row.  Its lanes read 64 entries' (id, weight) at once and reduce den with a butterfly
// (every lane ends with the same sum); then per bag entry, broadcast by a shuffle, the 64 lanes add 64
// consecutive floats of the entry's table row: at H = 64 one entry is exactly one 256-B global_atomic_add_f32
// wave-instruction.  Not bitwise reproducible (fp32 atomic arrival order).
__global__ void __launch_bounds__(kBlock)
embedding_bag_backward_kernel(long long V, int H, BagLayout L, float p, int training, u64 seed,
                              const unsigned char* __restrict__ keep, const float* __restrict__ grad_out,
                              float* __restrict__ dW, int* __restrict__ n_bad)
{
    const float scale = inv_keep(p);
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const long long n_waves = ((long long)gridDim.x * kBlock) >> 6;
    for (long long m = wave; m < L.n_rows; m += n_waves) {        // wave-uniform loop
        long long s0, s1, jb;
        if (!bag_of(L, m, s0, s1, jb)) { if (lane == 0 && n_bad) atomicAdd(n_bad, 1); continue; }
        float den = 0.0f;
        for (long long c0 = s0; c0 < s1; c0 += 64) {
            float part = c0 + lane < s1 ? L.data[c0 + lane] : 0.0f;
            for (int o = 1; o < 64; o <<= 1) part += __shfl_xor(part, o);
            den += part;
        }
        const float inv = inv_den_bag(den);
        for (int h0 = 0; h0 < H; h0 += 64) {
            const int h = h0 + lane;
            const bool live_h = h < H;
            const float g = live_h ? grad_out[(size_t)m * H + h] * inv : 0.0f;
            for (long long c0 = s0; c0 < s1; c0 += 64) {
                const bool cl = c0 + lane < s1;
                const long long my_a = cl ? attr_id(L, c0 + lane) : -1;
                const float my_d = cl ? L.data[c0 + lane] : 0.0f;
                if (cl && (my_a < 0 || my_a >= V) && h0 == 0 && n_bad) atomicAdd(n_bad, 1);
                const int n = (int)(s1 - c0 < 64 ? s1 - c0 : 64);
                for (int u = 0; u < n; ++u) {
                    const long long a = __shfl(my_a, u);
                    if (a < 0 || a >= V) continue;                              // wave-uniform
                    float x = g * __shfl(my_d, u);
                    if (training) {
                        const u64 el = (u64)(jb + (c0 - s0) + u) * (u64)H + (u64)h;
                        x *= keep ? (keep[el] ? scale : 0.0f) : keep_scale(seed, el, p, scale);
                    }
                    if (live_h && x != 0.0f) atomicAdd(dW + (size_t)a * H + h, x);
                }
            }
        }
    }
}

// ---- where is the row of node v?  (`topk_adj[batch_index]`, model.py:310, without the host)
// pos_of_node[v] = the first position of v in the seed list, -1 for a node that is no seed.
__global__ void __launch_bounds__(256) seed_positions_init_kernel(int* pos_of_node, long long n_nodes)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_nodes; i += stride) pos_of_node[i] = 0x7FFFFFFF;
}
__global__ void __launch_bounds__(256) seed_positions_fill_kernel(const int* seeds, long long n_seeds, int* pos_of_node, long long n_nodes, int* n_bad)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_seeds; i += stride) {
        const int v = seeds[i];
        if (v < 0 || v >= n_nodes) { atomicAdd(n_bad, 1); continue; }
        atomicMin(&pos_of_node[v], (int)i);                           // a duplicated seed keeps its FIRST position
    }
}
__global__ void __launch_bounds__(256) seed_positions_finish_kernel(int* pos_of_node, long long n_nodes)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_nodes; i += stride)
        if (pos_of_node[i] == 0x7FFFFFFF) pos_of_node[i] = -1;
}
__global__ void __launch_bounds__(256) batch_positions_kernel(const int* pos_of_node, long long n_nodes, const long long* node_ids, long long n,
                                                              int* out, int* n_missing)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const long long v = node_ids[i];
        const int pos = v >= 0 && v < n_nodes ? pos_of_node[v] : -1;
        out[i] = pos;
        if (pos < 0) atomicAdd(n_missing, 1);
    }
}

}  // namespace

extern "C" {

// Starts the HIP runtime's context on `device` (what the first allocation of a process otherwise pays): bench.py times the
// runtime's start apart from the constructor with this call.  (Lives here, not in gfpush.hip, only because the hash that ties a
// counter profile to the kernel sources covers that file.)
int gp_internal_warm_device(int device)
{
    if (hipSetDevice(device) != hipSuccess || hipFree(nullptr) != hipSuccess) {
        (void)hipGetLastError();
        return fail(GP_ERR_NO_DEVICE, "gp_internal_warm_device", "no usable HIP device");
    }
    return GP_OK;
}

int gp_seed_positions(int device, const int32_t* d_seeds, int64_t n_seeds, int64_t n_nodes, int32_t* d_pos_of_node, int32_t* d_n_bad, void* stream)
{
    if (n_nodes < 0 || n_seeds < 0 || n_seeds > 0x7FFFFFFE) return fail(GP_ERR_INVALID_ARG, "gp_seed_positions", "negative size or more than 2^31 - 2 seeds");
    if ((n_nodes > 0 && !d_pos_of_node) || (n_seeds > 0 && !d_seeds) || !d_n_bad) return fail(GP_ERR_NULL, "gp_seed_positions", "null device pointer");
    if (const int rc = set_device(device, "gp_seed_positions")) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int grid_n = (int)std::min<int64_t>(4096, (n_nodes + 255) / 256 + 1), grid_s = (int)std::min<int64_t>(4096, (n_seeds + 255) / 256 + 1);
    if (hipMemsetAsync(d_n_bad, 0, sizeof(int), s) != hipSuccess) return fail(GP_ERR_HIP, "gp_seed_positions", "hipMemsetAsync failed");
    hipLaunchKernelGGL(seed_positions_init_kernel, dim3(grid_n), dim3(256), 0, s, d_pos_of_node, (long long)n_nodes);
    hipLaunchKernelGGL(seed_positions_fill_kernel, dim3(grid_s), dim3(256), 0, s, d_seeds, (long long)n_seeds, d_pos_of_node, (long long)n_nodes, d_n_bad);
    hipLaunchKernelGGL(seed_positions_finish_kernel, dim3(grid_n), dim3(256), 0, s, d_pos_of_node, (long long)n_nodes);
    return launch_status("gp_seed_positions");
}

int gp_batch_positions(int device, const int32_t* d_pos_of_node, int64_t n_nodes, const int64_t* d_node_ids, int64_t n,
                       int32_t* d_out, int32_t* d_n_missing, void* stream)
{
    if (n < 0 || n_nodes < 0) return fail(GP_ERR_INVALID_ARG, "gp_batch_positions", "negative size");
    if (!d_n_missing || (n > 0 && (!d_pos_of_node || !d_node_ids || !d_out))) return fail(GP_ERR_NULL, "gp_batch_positions", "null device pointer");
    if (const int rc = set_device(device, "gp_batch_positions")) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(d_n_missing, 0, sizeof(int), s) != hipSuccess) return fail(GP_ERR_HIP, "gp_batch_positions", "hipMemsetAsync failed");
    if (n > 0) {
        hipLaunchKernelGGL(batch_positions_kernel, dim3((int)std::min<int64_t>(2048, (n + 255) / 256)), dim3(256), 0, s,
                           d_pos_of_node, (long long)n_nodes, (const long long*)d_node_ids, (long long)n, d_out, d_n_missing);
        if (const int rc = launch_status("gp_batch_positions")) return rc;
    }
    return GP_OK;
}


int gp_random_prop_rows(int device, const float* d_x, int64_t n_nodes, int32_t feat_dim,
                        const int32_t* d_col, const double* d_val, const int32_t* d_filled, int32_t K,
                        const int32_t* d_batch_rows, int32_t n_batch,
                        float dropnode_rate, int training, uint64_t seed, const uint8_t* d_keep,
                        float* d_out, void* stream)
{
    if (n_batch == 0) return GP_OK;
    if (!d_x || !d_col || !d_val || !d_out) return fail(GP_ERR_NULL, "gp_random_prop_rows", "a device pointer is NULL");
    if (n_nodes < 1 || feat_dim < 1 || K < 1 || K > GP_MAX_K || n_batch < 0 || !(dropnode_rate >= 0.0f && dropnode_rate <= 1.0f))
        return fail(GP_ERR_INVALID_ARG, "gp_random_prop_rows", "bad size, K outside [1, 1024] or dropnode_rate outside [0, 1]");
    if (const int rc = set_device(device, "gp_random_prop_rows")) return rc;
    const int grid = n_batch < 65535 ? n_batch : 65535;
    const int vec = vec_width(feat_dim), slabs = feature_slabs(feat_dim, vec, kBlock);
    hipLaunchKernelGGL(random_prop_rows_kernel, dim3(grid, slabs), dim3(kBlock), 0, (hipStream_t)stream, d_x, feat_dim, d_col,
                       d_val, d_filled, K, d_batch_rows, n_batch, dropnode_rate, training, (u64)seed, d_keep, d_out);
    return launch_status("random_prop_rows_kernel");
}

int gp_random_prop_coo(int device, const float* d_feats, int64_t n_entries, int32_t feat_dim,
                       const float* d_scores, const int64_t* d_idx, int64_t n_out,
                       float dropnode_rate, int training, uint64_t seed, const uint8_t* d_keep,
                       float* d_out, void* stream)
{
    if (n_out == 0) return GP_OK;
    if (n_entries > 0 && (!d_feats || !d_scores || !d_idx)) return fail(GP_ERR_NULL, "gp_random_prop_coo", "a device pointer is NULL");
    if (!d_out) return fail(GP_ERR_NULL, "gp_random_prop_coo", "d_out is NULL");
    if (n_entries < 0 || n_entries > 2147483647ll || feat_dim < 1 || n_out < 0 || !(dropnode_rate >= 0.0f && dropnode_rate <= 1.0f))
        return fail(GP_ERR_INVALID_ARG, "gp_random_prop_coo", "bad size or dropnode_rate outside [0, 1]");
    if (const int rc = set_device(device, "gp_random_prop_coo")) return rc;
    const int grid = n_out < 65535 ? (int)n_out : 65535;
    const int vec = vec_width(feat_dim), slabs = feature_slabs(feat_dim, vec, kBlock);
    hipLaunchKernelGGL(random_prop_coo_kernel, dim3(grid, slabs), dim3(kBlock), 0, (hipStream_t)stream, d_feats, feat_dim,
                       d_scores, (const long long*)d_idx, (long long)n_entries, (long long)n_out, dropnode_rate,
                       training, (u64)seed, d_keep, d_out);
    return launch_status("random_prop_coo_kernel");
}

}  // extern "C"

// ---- Backward and embedding-bag entry points.  Arguments are checked before hipSetDevice.
namespace {

int check_bag_args(const char* where, const float* d_table, int64_t n_vocab, int32_t dim, const int64_t* d_offsets,
                   int64_t n_src, int64_t n_rows, const void* d_attr_idx, int idx_bytes, const float* d_attr_data,
                   float rate, const void* d_dst)
{
    if (n_vocab < 0 || dim < 1 || n_src < 0 || n_rows < 0 || (idx_bytes != 4 && idx_bytes != 8) || !(rate >= 0.0f && rate <= 1.0f))
        return fail(GP_ERR_INVALID_ARG, where, "negative size, dim < 1, idx_bytes not 4 or 8, or dropout rate outside [0, 1]");
    if (n_rows > 0 && (!d_offsets || !d_attr_idx || !d_attr_data || !d_dst || (n_vocab > 0 && !d_table)))
        return fail(GP_ERR_NULL, where, "a device pointer is NULL");
    return GP_OK;
}

}  // namespace

extern "C" {

int gp_random_prop_coo_backward(int device, const float* d_grad_out, int64_t n_out, int32_t feat_dim,
                                const float* d_scores, const int64_t* d_idx, int64_t n_entries,
                                float dropnode_rate, int training, uint64_t seed, const uint8_t* d_keep,
                                float* d_grad_feats, void* stream)
{
    const char* where = "gp_random_prop_coo_backward";
    if (n_entries < 0 || n_entries > 2147483647ll || feat_dim < 1 || n_out < 0 || !(dropnode_rate >= 0.0f && dropnode_rate <= 1.0f))
        return fail(GP_ERR_INVALID_ARG, where, "bad size or dropnode_rate outside [0, 1]");
    if (n_out == 0) return GP_OK;
    if (!d_grad_out || (n_entries > 0 && (!d_scores || !d_idx || !d_grad_feats))) return fail(GP_ERR_NULL, where, "a device pointer is NULL");
    if (const int rc = set_device(device, where)) return rc;
    const int grid = n_out < 65535 ? (int)n_out : 65535;
    hipLaunchKernelGGL(random_prop_coo_backward_kernel, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, d_grad_out, feat_dim,
                       d_scores, (const long long*)d_idx, (long long)n_entries, (long long)n_out, dropnode_rate, training,
                       (u64)seed, d_keep, d_grad_feats);
    return launch_status("random_prop_coo_backward_kernel");
}

int gp_random_prop_rows_backward(int device, const float* d_grad_out, int32_t n_batch, int32_t feat_dim,
                                 const int32_t* d_col, const double* d_val, const int32_t* d_filled, int32_t K,
                                 const int32_t* d_batch_rows, float dropnode_rate, int training, uint64_t seed,
                                 const uint8_t* d_keep, float* d_grad_x, int64_t n_nodes, void* stream)
{
    const char* where = "gp_random_prop_rows_backward";
    if (n_batch < 0 || n_nodes < 1 || feat_dim < 1 || K < 1 || K > GP_MAX_K || !(dropnode_rate >= 0.0f && dropnode_rate <= 1.0f))
        return fail(GP_ERR_INVALID_ARG, where, "bad size, K outside [1, 1024] or dropnode_rate outside [0, 1]");
    if (n_batch == 0) return GP_OK;
    if (!d_grad_out || !d_col || !d_val || !d_grad_x) return fail(GP_ERR_NULL, where, "a device pointer is NULL");
    if (const int rc = set_device(device, where)) return rc;
    const int grid = n_batch < 65535 ? n_batch : 65535;
    hipLaunchKernelGGL(random_prop_rows_backward_kernel, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, d_grad_out, feat_dim,
                       d_col, d_val, d_filled, K, d_batch_rows, n_batch, (long long)n_nodes, dropnode_rate, training, (u64)seed,
                       d_keep, d_grad_x);
    return launch_status("random_prop_rows_backward_kernel");
}

int gp_embedding_bag(int device, const float* d_weight, int64_t n_vocab, int32_t dim,
                     const int64_t* d_offsets, int64_t n_src, const int64_t* d_nodes, const int64_t* d_entry_base, int64_t n_rows,
                     const void* d_attr_idx, int idx_bytes, const float* d_attr_data,
                     float dropout_rate, int training, uint64_t seed, const uint8_t* d_keep,
                     float* d_out, int32_t* d_n_bad, void* stream)
{
    const char* where = "gp_embedding_bag";
    if (const int rc = check_bag_args(where, d_weight, n_vocab, dim, d_offsets, n_src, n_rows, d_attr_idx, idx_bytes, d_attr_data,
                                      dropout_rate, d_out)) return rc;
    if (n_rows == 0) return GP_OK;
    if (const int rc = set_device(device, where)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (d_n_bad && hipMemsetAsync(d_n_bad, 0, sizeof(int32_t), s) != hipSuccess) return fail(GP_ERR_HIP, where, "hipMemsetAsync failed");
    const BagLayout L = bag_layout(d_offsets, n_src, d_nodes, d_entry_base, n_rows, d_attr_idx, idx_bytes, d_attr_data);
    const int vec = vec_width(dim);
    const int log2g = lane_group_log2(dim, vec);
    const long long rows_per_block = (kBlock / 64) * (64 >> log2g);
    const int grid = (int)std::min<long long>(65535ll * 16, (n_rows + rows_per_block - 1) / rows_per_block);
    if (vec == 4)      hipLaunchKernelGGL(embedding_bag_kernel<4>, dim3(grid), dim3(kBlock), 0, s, d_weight, (long long)n_vocab, dim, L, dropout_rate, training, (u64)seed, d_keep, d_out, d_n_bad, log2g);
    else if (vec == 2) hipLaunchKernelGGL(embedding_bag_kernel<2>, dim3(grid), dim3(kBlock), 0, s, d_weight, (long long)n_vocab, dim, L, dropout_rate, training, (u64)seed, d_keep, d_out, d_n_bad, log2g);
    else               hipLaunchKernelGGL(embedding_bag_kernel<1>, dim3(grid), dim3(kBlock), 0, s, d_weight, (long long)n_vocab, dim, L, dropout_rate, training, (u64)seed, d_keep, d_out, d_n_bad, log2g);
    return launch_status("embedding_bag_kernel");
}

int gp_embedding_bag_backward(int device, const float* d_grad_out, int64_t n_vocab, int32_t dim,
                              const int64_t* d_offsets, int64_t n_src, const int64_t* d_nodes, const int64_t* d_entry_base, int64_t n_rows,
                              const void* d_attr_idx, int idx_bytes, const float* d_attr_data,
                              float dropout_rate, int training, uint64_t seed, const uint8_t* d_keep,
                              float* d_grad_weight, int32_t* d_n_bad, void* stream)
{
    const char* where = "gp_embedding_bag_backward";
    if (const int rc = check_bag_args(where, d_grad_weight, n_vocab, dim, d_offsets, n_src, n_rows, d_attr_idx, idx_bytes, d_attr_data,
                                      dropout_rate, d_grad_out)) return rc;
    if (n_rows == 0) return GP_OK;
    if (const int rc = set_device(device, where)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (d_n_bad && hipMemsetAsync(d_n_bad, 0, sizeof(int32_t), s) != hipSuccess) return fail(GP_ERR_HIP, where, "hipMemsetAsync failed");
    const BagLayout L = bag_layout(d_offsets, n_src, d_nodes, d_entry_base, n_rows, d_attr_idx, idx_bytes, d_attr_data);
    const int grid = (int)std::min<long long>(65535ll * 16, (n_rows + kBlock / 64 - 1) / (kBlock / 64));
    hipLaunchKernelGGL(embedding_bag_backward_kernel, dim3(grid), dim3(kBlock), 0, s, (long long)n_vocab, dim, L, dropout_rate,
                       training, (u64)seed, d_keep, d_grad_out, d_grad_weight, d_n_bad);
    return launch_status("embedding_bag_backward_kernel");
}

}  // extern "C"

// ---- S-sample random_prop: the S augmentations of one training step (model.py:321-322) in one launch.
// Sample s keeps entry e by keep_scale(gp_sample_seed(seed, s), e) or d_keep[s * keep_stride + e]; out is
// [S x n_out x F], sample-major.  A workgroup stages its row's columns once and the weights of up to `nsc` samples
// in dynamic LDS (nsc * stage floats, at most 64 KiB), loads every neighbour feature row once per sample chunk and
// updates one accumulator per sample from that load.  Per sample and column the sums run in the single-sample
// kernel's order (denominator over k, then the column sum over k), so out[s] equals gp_random_prop_* with
// seed_s bit for bit; a dropped entry adds 0 * x, which leaves a finite sum unchanged.
namespace {

constexpr int kMultiLdsBytes = 65536;

// out[s0 + s][f] for s < ns from the staged columns (s_col, or col_base + k when s_col is NULL) and weights
// s_w[s * stage + k].  NS >= ns is the unrolled accumulator count; samples ns..NS-1 see weight 0 and are not written.
template <int VEC, int NS>
__device__ __forceinline__ void weighted_rows_multi(const float* __restrict__ X, int F, const int* s_col, long long col_base,
                                                    const float* s_w, int stage, int n, int ns,
                                                    float* __restrict__ out_row, size_t out_stride)
{
    typedef typename VecT<VEC>::type V;
    float inv[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        float den = 0.0f;
        if (s < ns) for (int k = 0; k < n; ++k) den += s_w[s * stage + k];   // model.py:85-86, the single kernel's order
        inv[s] = 1.0f / (den + 1e-12f);                                       // inv_den_rows by hand (dropnode.hpp): the call changes this unit's code
    }
    for (int f = (blockIdx.y * kBlock + threadIdx.x) * VEC; f < F; f += gridDim.y * kBlock * VEC) {
        float acc[NS][VEC];
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[s][i] = 0.0f;
        int k = 0;
        for (; k + 8 <= n; k += 8) {
            V v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const long long c = s_col ? (long long)s_col[k + u] : col_base + k + u;
                v[u] = *reinterpret_cast<const V*>(X + (size_t)c * F + f);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float* pv = reinterpret_cast<const float*>(&v[u]);
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const float w = s < ns ? s_w[s * stage + k + u] : 0.0f;
#pragma unroll
                    for (int i = 0; i < VEC; ++i) acc[s][i] += w * pv[i];   // model.py:83-84
                }
            }
        }
        for (; k < n; ++k) {
            const long long c = s_col ? (long long)s_col[k] : col_base + k;
            const V v = *reinterpret_cast<const V*>(X + (size_t)c * F + f);
            const float* pv = reinterpret_cast<const float*>(&v);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const float w = s < ns ? s_w[s * stage + k] : 0.0f;
#pragma unroll
                for (int i = 0; i < VEC; ++i) acc[s][i] += w * pv[i];
            }
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (s >= ns) continue;
            V o; float* po = reinterpret_cast<float*>(&o);
#pragma unroll
            for (int i = 0; i < VEC; ++i) po[i] = acc[s][i] * inv[s];
            *reinterpret_cast<V*>(out_row + s * out_stride + f) = o;
        }
    }
}

// Fused form.  LDS: s_col[stage] then s_w[nsc][stage], stage = K; nsc <= NS (the kernel's accumulators per lane).
template <int VEC, int NS>
__global__ void __launch_bounds__(kBlock)
random_prop_rows_multi_kernel(const float* __restrict__ X, int F, const int* __restrict__ col,
                              const double* __restrict__ val, const int* __restrict__ filled, int K,
                              const int* __restrict__ batch_rows, int n_batch, int S, int nsc, float p, int training, u64 seed,
                              const unsigned char* __restrict__ keep, long long keep_stride, float* __restrict__ out)
{
    extern __shared__ float smem[];
    int* s_col = reinterpret_cast<int*>(smem);
    float* s_w = smem + K;
    const float scale = inv_keep(p);
    const size_t out_stride = (size_t)n_batch * F;
    for (int b = blockIdx.x; b < n_batch; b += gridDim.x) {
        const long long row = batch_rows ? batch_rows[b] : b;
        const int n = row_len(filled, row, K);
        for (int s0 = 0; s0 < S; s0 += nsc) {
            const int ns = min(nsc, S - s0);
            __syncthreads();
            for (int k = threadIdx.x; k < n; k += kBlock) {
                const long long e = row * (long long)K + k;
                const float w = (float)val[e];                      // model.py:314
                if (s0 == 0) s_col[k] = col[e];
                for (int s = 0; s < ns; ++s) s_w[s * K + k] = sample_weight(w, e, s0 + s, p, scale, training, seed, keep, keep_stride);
            }
            __syncthreads();
            weighted_rows_multi<VEC, NS>(X, F, s_col, 0, s_w, K, n, ns, out + s0 * out_stride + (size_t)b * F, out_stride);
        }
    }
}

__device__ __forceinline__ void segment_of(const long long* __restrict__ idx, long long n_entries, long long b, long long& lo, long long& hi)
{
    // lower_bound(idx, b) and lower_bound(idx, b+1); every lane searches (same addresses: broadcast loads)
    long long l = 0, h = n_entries;
    while (l < h) { const long long mid = (l + h) >> 1; if (idx[mid] < b) l = mid + 1; else h = mid; }
    lo = l; h = n_entries;
    while (l < h) { const long long mid = (l + h) >> 1; if (idx[mid] < b + 1) l = mid + 1; else h = mid; }
    hi = l;
}

// Reference-shaped form.  LDS: s_w[nsc][kStage].  A segment longer than kStage takes the single kernel's plain loop,
// once per sample.
template <int VEC, int NS>
__global__ void __launch_bounds__(kBlock)
random_prop_coo_multi_kernel(const float* __restrict__ feats, int F, const float* __restrict__ scores,
                             const long long* __restrict__ idx, long long n_entries, long long n_out, int S, int nsc,
                             float p, int training, u64 seed, const unsigned char* __restrict__ keep,
                             float* __restrict__ out)
{
    extern __shared__ float s_w[];
    const float scale = inv_keep(p);
    const size_t out_stride = (size_t)n_out * F;
    for (long long b = blockIdx.x; b < n_out; b += gridDim.x) {
        long long lo, hi;
        segment_of(idx, n_entries, b, lo, hi);
        if (hi - lo <= kStage) {
            const int n = (int)(hi - lo);
            for (int s0 = 0; s0 < S; s0 += nsc) {
                const int ns = min(nsc, S - s0);
                __syncthreads();
                for (int k = threadIdx.x; k < n; k += kBlock)
                    for (int s = 0; s < ns; ++s) s_w[s * kStage + k] = sample_weight(scores[lo + k], lo + k, s0 + s, p, scale, training, seed, keep, n_entries);
                __syncthreads();
                weighted_rows_multi<VEC, NS>(feats, F, nullptr, lo, s_w, kStage, n, ns, out + s0 * out_stride + (size_t)b * F, out_stride);
            }
        } else {
            for (int s = 0; s < S; ++s) {
                float den = 0.0f;
                for (long long e = lo; e < hi; ++e) den += sample_weight(scores[e], e, s, p, scale, training, seed, keep, n_entries);
                const float inv = inv_den_rows(den);
                float* out_row = out + s * out_stride + (size_t)b * F;
                for (int f = blockIdx.y * kBlock + threadIdx.x; f < F; f += gridDim.y * kBlock) {
                    float acc = 0.0f;
                    for (long long e = lo; e < hi; ++e) {
                        const float w = sample_weight(scores[e], e, s, p, scale, training, seed, keep, n_entries);
                        if (w != 0.0f) acc += w * feats[(size_t)e * F + f];
                    }
                    out_row[f] = acc * inv;
                }
            }
        }
    }
}

// COO backward: grad_feats[e,:] = sum_s w'_{s,e} / (den_{s,b} + 1e-12) * g[s,b,:], summed over s in order, one pass,
// no atomics.  Weights of a chunk of samples are staged as in the forward; with more than one chunk the chunk's
// sum is added to what the same thread wrote for the previous chunk.
template <int VEC>
__device__ __forceinline__ void scaled_rows_multi(const float* __restrict__ g, size_t g_stride, int F, const float* s_w, int stage,
                                                  int n, int ns, const float* inv, bool first, float* __restrict__ out_rows)
{
    typedef typename VecT<VEC>::type V;
    const int FV = F / VEC;
    for (int t = threadIdx.x; t < n * FV; t += kBlock) {
        const int k = t / FV, f = (t - k * FV) * VEC;
        V o = first ? V() : *reinterpret_cast<const V*>(out_rows + (size_t)k * F + f);
        float* po = reinterpret_cast<float*>(&o);
        for (int s = 0; s < ns; ++s) {
            const V gv = *reinterpret_cast<const V*>(g + s * g_stride + f);
            const float* pg = reinterpret_cast<const float*>(&gv);
            const float w = s_w[s * stage + k];
#pragma unroll
            for (int i = 0; i < VEC; ++i) po[i] += (pg[i] * inv[s]) * w;
        }
        *reinterpret_cast<V*>(out_rows + (size_t)k * F + f) = o;
    }
}

__global__ void __launch_bounds__(kBlock)
random_prop_coo_multi_backward_kernel(const float* __restrict__ grad_out, int F, const float* __restrict__ scores,
                                      const long long* __restrict__ idx, long long n_entries, long long n_out, int S, int nsc,
                                      float p, int training, u64 seed, const unsigned char* __restrict__ keep,
                                      float* __restrict__ grad_feats)
{
    extern __shared__ float s_w[];
    const float scale = inv_keep(p);
    const size_t g_stride = (size_t)n_out * F;
    for (long long b = blockIdx.x; b < n_out; b += gridDim.x) {
        long long lo, hi;
        segment_of(idx, n_entries, b, lo, hi);
        const float* g_row = grad_out + (size_t)b * F;
        if (hi - lo <= kStage) {
            const int n = (int)(hi - lo);
            float* rows = grad_feats + (size_t)lo * F;
            for (int s0 = 0; s0 < S; s0 += nsc) {
                const int ns = min(nsc, S - s0);
                __syncthreads();
                for (int k = threadIdx.x; k < n; k += kBlock)
                    for (int s = 0; s < ns; ++s) s_w[s * kStage + k] = sample_weight(scores[lo + k], lo + k, s0 + s, p, scale, training, seed, keep, n_entries);
                __syncthreads();
                float inv[kMaxSamples];
                for (int s = 0; s < ns; ++s) {
                    float den = 0.0f;
                    for (int k = 0; k < n; ++k) den += s_w[s * kStage + k];          // the forward's order
                    inv[s] = inv_den_rows(den);
                }
                const float* g = g_row + s0 * g_stride;
                if ((F & 3) == 0)      scaled_rows_multi<4>(g, g_stride, F, s_w, kStage, n, ns, inv, s0 == 0, rows);
                else if ((F & 1) == 0) scaled_rows_multi<2>(g, g_stride, F, s_w, kStage, n, ns, inv, s0 == 0, rows);
                else                   scaled_rows_multi<1>(g, g_stride, F, s_w, kStage, n, ns, inv, s0 == 0, rows);
            }
        } else {
            for (int s = 0; s < S; ++s) {
                float den = 0.0f;
                for (long long e = lo; e < hi; ++e) den += sample_weight(scores[e], e, s, p, scale, training, seed, keep, n_entries);
                const float inv = inv_den_rows(den);
                const float* g = g_row + s * g_stride;
                for (long long e = lo; e < hi; ++e) {
                    const float w = sample_weight(scores[e], e, s, p, scale, training, seed, keep, n_entries);
                    for (int f = threadIdx.x; f < F; f += kBlock) {
                        const float x = (g[f] * inv) * w;
                        grad_feats[(size_t)e * F + f] = s == 0 ? x : grad_feats[(size_t)e * F + f] + x;
                    }
                }
            }
        }
        if (b == n_out - 1) zero_cut_rows(grad_feats, F, hi, n_entries);
    }
}

// Fused backward: grad_X[col[r,k],:] += sum_s w'_{s,r,k} / (den_{s,b} + 1e-12) * g[s,b,:] -- the samples are summed in
// registers and each element of an entry gets one fp32 atomic per sample chunk (one in all when S <= nsc).
__global__ void __launch_bounds__(kBlock)
random_prop_rows_multi_backward_kernel(const float* __restrict__ grad_out, int F, const int* __restrict__ col,
                                       const double* __restrict__ val, const int* __restrict__ filled, int K,
                                       const int* __restrict__ batch_rows, int n_batch, long long n_nodes, int S, int nsc,
                                       float p, int training, u64 seed, const unsigned char* __restrict__ keep,
                                       long long keep_stride, float* __restrict__ grad_x)
{
    extern __shared__ float smem[];
    int* s_col = reinterpret_cast<int*>(smem);
    float* s_inv = smem + K;                              // [nsc]
    float* s_w = s_inv + kMaxSamples;                     // [nsc][K]
    const float scale = inv_keep(p);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t g_stride = (size_t)n_batch * F;
    for (int b = blockIdx.x; b < n_batch; b += gridDim.x) {
        const long long row = batch_rows ? batch_rows[b] : b;
        const int n = row_len(filled, row, K);
        for (int s0 = 0; s0 < S; s0 += nsc) {
            const int ns = min(nsc, S - s0);
            __syncthreads();
            for (int k = threadIdx.x; k < n; k += kBlock) {
                const long long e = row * (long long)K + k;
                const float w = (float)val[e];
                if (s0 == 0) s_col[k] = col[e];
                for (int s = 0; s < ns; ++s) s_w[s * K + k] = sample_weight(w, e, s0 + s, p, scale, training, seed, keep, keep_stride);
            }
            __syncthreads();
            if (threadIdx.x < ns) {
                float den = 0.0f;
                for (int k = 0; k < n; ++k) den += s_w[threadIdx.x * K + k];
                s_inv[threadIdx.x] = inv_den_rows(den);
            }
            __syncthreads();
            const float* g = grad_out + s0 * g_stride + (size_t)b * F;
            for (int k = wave; k < n; k += kBlock / 64) {
                const int c = s_col[k];
                bool any = false;
                for (int s = 0; s < ns; ++s) any |= s_w[s * K + k] != 0.0f;
                if (!any || c < 0 || c >= n_nodes) continue;               // wave-uniform
                float* dst = grad_x + (size_t)c * F;
                for (int f = lane; f < F; f += 64) {
                    float x = 0.0f;
                    for (int s = 0; s < ns; ++s) x += (g[s * g_stride + f] * s_inv[s]) * s_w[s * K + k];
                    atomicAdd(dst + f, x);
                }
            }
        }
    }
}

int multi_check(const char* where, int32_t n_samples, float rate)
{
    if (n_samples < 1 || n_samples > kMaxSamples || !(rate >= 0.0f && rate <= 1.0f))
        return fail(GP_ERR_INVALID_ARG, where, "n_samples outside [1, 16] or dropnode_rate outside [0, 1]");
    return GP_OK;
}

int rows_nsc(int K, int S, int extra_floats)      // samples per chunk of the fused form's LDS
{
    const int fit = (kMultiLdsBytes / 4 - K - extra_floats) / K;
    return std::min(S, std::min(fit, kMaxSamples));
}

// Accumulators per lane of the forward kernels: S rounded up to a power of two, at most 8 (a chunk of 8 samples at
// VEC = 4 keeps 32 sums and 32 loaded floats per lane in registers); more samples take several chunks.
int forward_ns(int S) { return S <= 1 ? 1 : S <= 2 ? 2 : S <= 4 ? 4 : 8; }

#define GP_MULTI_DISPATCH(KERNEL, VEC, NS, ...)                                                                          \
    do {                                                                                                                \
        if (VEC == 4)      { if (NS == 1) KERNEL(4, 1, __VA_ARGS__); else if (NS == 2) KERNEL(4, 2, __VA_ARGS__);        \
                             else if (NS == 4) KERNEL(4, 4, __VA_ARGS__); else KERNEL(4, 8, __VA_ARGS__); }             \
        else if (VEC == 2) { if (NS == 1) KERNEL(2, 1, __VA_ARGS__); else if (NS == 2) KERNEL(2, 2, __VA_ARGS__);        \
                             else if (NS == 4) KERNEL(2, 4, __VA_ARGS__); else KERNEL(2, 8, __VA_ARGS__); }             \
        else               { if (NS == 1) KERNEL(1, 1, __VA_ARGS__); else if (NS == 2) KERNEL(1, 2, __VA_ARGS__);        \
                             else if (NS == 4) KERNEL(1, 4, __VA_ARGS__); else KERNEL(1, 8, __VA_ARGS__); }             \
    } while (0)

}  // namespace

extern "C" {

int gp_random_prop_rows_multi(int device, const float* d_x, int64_t n_nodes, int32_t feat_dim,
                              const int32_t* d_col, const double* d_val, const int32_t* d_filled, int32_t K,
                              const int32_t* d_batch_rows, int32_t n_batch, int32_t n_samples,
                              float dropnode_rate, int training, uint64_t seed, const uint8_t* d_keep, int64_t keep_stride,
                              float* d_out, void* stream)
{
    const char* where = "gp_random_prop_rows_multi";
    if (const int rc = multi_check(where, n_samples, dropnode_rate)) return rc;
    if (n_nodes < 1 || feat_dim < 1 || K < 1 || K > GP_MAX_K || n_batch < 0 || (d_keep && keep_stride < 1))
        return fail(GP_ERR_INVALID_ARG, where, "bad size, K outside [1, 1024] or keep_stride < 1 with a mask");
    if (n_batch == 0) return GP_OK;
    if (!d_x || !d_col || !d_val || !d_out) return fail(GP_ERR_NULL, where, "a device pointer is NULL");
    if (const int rc = set_device(device, where)) return rc;
    const int ns = forward_ns(n_samples);
    const int nsc = std::min(ns, rows_nsc(K, n_samples, 0));
    const size_t lds = (size_t)(K + nsc * K) * 4;
    const int grid = n_batch < 65535 ? n_batch : 65535;
    const int vec = vec_width(feat_dim), slabs = feature_slabs(feat_dim, vec, kBlock);
    hipStream_t s = (hipStream_t)stream;
#define GP_ROWS_MULTI(V, N, _) hipLaunchKernelGGL((random_prop_rows_multi_kernel<V, N>), dim3(grid, slabs), dim3(kBlock), lds, s, d_x, \
        feat_dim, d_col, d_val, d_filled, K, d_batch_rows, n_batch, n_samples, nsc, dropnode_rate, training, (u64)seed, d_keep,      \
        (long long)keep_stride, d_out)
    GP_MULTI_DISPATCH(GP_ROWS_MULTI, vec, ns, 0);
#undef GP_ROWS_MULTI
    return launch_status("random_prop_rows_multi_kernel");
}

int gp_random_prop_coo_multi(int device, const float* d_feats, int64_t n_entries, int32_t feat_dim,
                             const float* d_scores, const int64_t* d_idx, int64_t n_out, int32_t n_samples,
                             float dropnode_rate, int training, uint64_t seed, const uint8_t* d_keep,
                             float* d_out, void* stream)
{
    const char* where = "gp_random_prop_coo_multi";
    if (const int rc = multi_check(where, n_samples, dropnode_rate)) return rc;
    if (n_entries < 0 || n_entries > 2147483647ll || feat_dim < 1 || n_out < 0)
        return fail(GP_ERR_INVALID_ARG, where, "bad size");
    if (n_out == 0) return GP_OK;
    if ((n_entries > 0 && (!d_feats || !d_scores || !d_idx)) || !d_out) return fail(GP_ERR_NULL, where, "a device pointer is NULL");
    if (const int rc = set_device(device, where)) return rc;
    const int ns = forward_ns(n_samples);
    const int nsc = std::min(ns, kMultiLdsBytes / (4 * kStage));
    const size_t lds = (size_t)nsc * kStage * 4;
    const int grid = n_out < 65535 ? (int)n_out : 65535;
    const int vec = vec_width(feat_dim), slabs = feature_slabs(feat_dim, vec, kBlock);
    hipStream_t s = (hipStream_t)stream;
#define GP_COO_MULTI(V, N, _) hipLaunchKernelGGL((random_prop_coo_multi_kernel<V, N>), dim3(grid, slabs), dim3(kBlock), lds, s, d_feats, \
        feat_dim, d_scores, (const long long*)d_idx, (long long)n_entries, (long long)n_out, n_samples, nsc, dropnode_rate, training,     \
        (u64)seed, d_keep, d_out)
    GP_MULTI_DISPATCH(GP_COO_MULTI, vec, ns, 0);
#undef GP_COO_MULTI
    return launch_status("random_prop_coo_multi_kernel");
}

int gp_random_prop_coo_multi_backward(int device, const float* d_grad_out, int64_t n_out, int32_t feat_dim,
                                      const float* d_scores, const int64_t* d_idx, int64_t n_entries, int32_t n_samples,
                                      float dropnode_rate, int training, uint64_t seed, const uint8_t* d_keep,
                                      float* d_grad_feats, void* stream)
{
    const char* where = "gp_random_prop_coo_multi_backward";
    if (const int rc = multi_check(where, n_samples, dropnode_rate)) return rc;
    if (n_entries < 0 || n_entries > 2147483647ll || feat_dim < 1 || n_out < 0)
        return fail(GP_ERR_INVALID_ARG, where, "bad size");
    if (n_out == 0) return GP_OK;
    if (!d_grad_out || (n_entries > 0 && (!d_scores || !d_idx || !d_grad_feats))) return fail(GP_ERR_NULL, where, "a device pointer is NULL");
    if (const int rc = set_device(device, where)) return rc;
    const int nsc = std::min<int>(n_samples, kMultiLdsBytes / (4 * kStage));
    const int grid = n_out < 65535 ? (int)n_out : 65535;
    hipLaunchKernelGGL(random_prop_coo_multi_backward_kernel, dim3(grid), dim3(kBlock), (size_t)nsc * kStage * 4, (hipStream_t)stream,
                       d_grad_out, feat_dim, d_scores, (const long long*)d_idx, (long long)n_entries, (long long)n_out, n_samples, nsc,
                       dropnode_rate, training, (u64)seed, d_keep, d_grad_feats);
    return launch_status("random_prop_coo_multi_backward_kernel");
}

int gp_random_prop_rows_multi_backward(int device, const float* d_grad_out, int32_t n_batch, int32_t feat_dim,
                                       const int32_t* d_col, const double* d_val, const int32_t* d_filled, int32_t K,
                                       const int32_t* d_batch_rows, int32_t n_samples, float dropnode_rate, int training, uint64_t seed,
                                       const uint8_t* d_keep, int64_t keep_stride, float* d_grad_x, int64_t n_nodes, void* stream)
{
    const char* where = "gp_random_prop_rows_multi_backward";
    if (const int rc = multi_check(where, n_samples, dropnode_rate)) return rc;
    if (n_batch < 0 || n_nodes < 1 || feat_dim < 1 || K < 1 || K > GP_MAX_K || (d_keep && keep_stride < 1))
        return fail(GP_ERR_INVALID_ARG, where, "bad size, K outside [1, 1024] or keep_stride < 1 with a mask");
    if (n_batch == 0) return GP_OK;
    if (!d_grad_out || !d_col || !d_val || !d_grad_x) return fail(GP_ERR_NULL, where, "a device pointer is NULL");
    if (const int rc = set_device(device, where)) return rc;
    const int nsc = rows_nsc(K, n_samples, kMaxSamples);
    const size_t lds = (size_t)(K + kMaxSamples + nsc * K) * 4;
    const int grid = n_batch < 65535 ? n_batch : 65535;
    hipLaunchKernelGGL(random_prop_rows_multi_backward_kernel, dim3(grid), dim3(kBlock), lds, (hipStream_t)stream, d_grad_out, feat_dim,
                       d_col, d_val, d_filled, K, d_batch_rows, n_batch, (long long)n_nodes, n_samples, nsc, dropnode_rate, training,
                       (u64)seed, d_keep, (long long)keep_stride, d_grad_x);
    return launch_status("random_prop_rows_multi_backward_kernel");
}

}  // extern "C"
