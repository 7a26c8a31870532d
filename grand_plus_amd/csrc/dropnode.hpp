// dropnode.hpp -- the DropNode weight, the embedding bag's layout and the two denominators of the training step's front
// end, defined once for augment.hip (§7d, §7e), scatter_det.hip (§7i), mag_prop.hip (§7k) and mag_det.hip (§7o).  They promise each
// other's bits; they keep the promise by calling the same lines:
//     scatter_det.hip's deterministic backwards give what augment.hip's atomic backwards give, up to the order of the sum:
//         the backward must find an entry, its bag, its mask and its denominator exactly as the forward finds them;
//     mag_prop.hip's rows carry random_prop_rows(samples = S)'s DropNode mask for the same seed;
//     out[s] of an S-sample call equals the single-sample call with gp_sample_seed(seed, s), bit for bit.
// A `+ 1e-12f` written out in a kernel is inv_den_rows by hand: there the call changed the unit's code.
// Everything has internal linkage, as in gp_common.hpp.
#pragma once

#include "gp_common.hpp"

namespace {

constexpr int kMaxSamples = 16;       // samples of one call (GP_MAX_SAMPLES of _native.py)
constexpr int kStage = 1024;          // most neighbours of one output row staged per pass
static_assert(kStage == GP_MAX_K, "a resident row fits one LDS stage");

// 1 / (1 - p), what a kept element is scaled by at rate p: F.dropout (model.py:82, model_mag.py:50); p = 1 keeps nothing
__device__ __forceinline__ float inv_keep(float p) { return p < 1.0f ? 1.0f / (1.0f - p) : 0.0f; }

// entries of resident row `row`: filled[row] capped at K, K without `filled`.  mag_prop.hip also clamps a negative
// filled[row] to 0 and keeps its own expression for that: the two differ there.
__device__ __forceinline__ int row_len(const int* __restrict__ filled, long long row, int K) { return filled ? min(filled[row], K) : K; }

__device__ __forceinline__ float inv_den_rows(float den) { return 1.0f / (den + 1e-12f); }   // model.py:87, model_mag.py:86
__device__ __forceinline__ float inv_den_bag(float den) { return 1.0f / (den + 1e-10f); }    // model_mag.py:54

// weight of entry e (raw weight w) in sample s: w itself in eval, else w * keep * scale, keep from d_keep[s * keep_stride + e]
// or from the hash of (gp_sample_seed(seed, s), e); scale = inv_keep(p)
__device__ __forceinline__ float sample_weight(float w, long long e, int s, float p, float scale, int training, u64 seed,
                                               const unsigned char* keep, long long keep_stride)
{
    if (!training) return w;
    return w * (keep ? (keep[(long long)s * keep_stride + e] ? scale : 0.0f) : keep_scale(sample_seed(seed, s), (u64)e, p, scale));
}

// ---- Embedding-bag (MAG's sparse first layer, MLP.emb, model_mag.py:48-55):
//     out[m, :] = sum_j keep_{j,:} s d_j W[a_j, :] / (sum_j d_j + 1e-10)
// Bag of output row m: storage entries [offsets[src], offsets[src + 1]) of (attr_idx, attr_data), src = nodes[m]
// (nodes != NULL: rows of a device-resident node-attribute CSR) or m.  j = entry_base[m] + t (entry_base != NULL)
// or the storage position itself: the entry's position in the batch's entry order, which keys the dropout of
// element (j, h) as (seed, j*H + h).  Attribute ids outside [0, V) are never read or written; they add to *n_bad.
struct BagLayout {
    const long long* offsets; long long n_src;        // offsets[n_src + 1]
    const long long* nodes;                             // [n_rows] or NULL
    const long long* base;                              // [n_rows] or NULL
    long long n_rows;
    const void* idx; int idx64;                         // attr ids: int64 (idx64) or int32
    const float* data;
};

__device__ __forceinline__ bool bag_of(const BagLayout& L, long long m, long long& s0, long long& s1, long long& jb)
{
    const long long src = L.nodes ? L.nodes[m] : m;
    if (src < 0 || src >= L.n_src) { s0 = s1 = jb = 0; return false; }
    s0 = L.offsets[src]; s1 = L.offsets[src + 1];
    jb = L.base ? L.base[m] : s0;
    return true;
}

__device__ __forceinline__ long long attr_id(const BagLayout& L, long long e)
{
    return L.idx64 ? reinterpret_cast<const long long*>(L.idx)[e] : (long long)reinterpret_cast<const int*>(L.idx)[e];
}

// host: the layout of an entry point's bag arguments
inline BagLayout bag_layout(const int64_t* d_offsets, int64_t n_src, const int64_t* d_nodes, const int64_t* d_entry_base,
                            int64_t n_rows, const void* d_attr_idx, int idx_bytes, const float* d_attr_data)
{
    return {(const long long*)d_offsets, (long long)n_src, (const long long*)d_nodes, (const long long*)d_entry_base,
            (long long)n_rows, d_attr_idx, idx_bytes == 8, d_attr_data};
}

}  // namespace
