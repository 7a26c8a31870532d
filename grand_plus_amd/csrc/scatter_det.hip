// scatter_det.hip -- DESIGN §7i: the two scatter backwards of augment.hip (random_prop_rows, embedding bag) without
// atomics on the gradient, so that it is bitwise the same run to run.  Sort-then-gather: the caller orders the entries
// of the call by destination row with a stable sort (plumbing, torch.sort); gather_sum_kernel below sums every
// destination row that occurs sequentially in that order, from 0.0f, and writes it once with plain stores.
//
// Order contract (include/grandplus_scatter.h states it in full; tests/test_gpu_deterministic_backward.py pins it):
//   rows form      entry e = b*K + k (b = position in the batch), contribution
//                  c_e[f] = sum_{s in order, from 0.0f} (g[s,b,f] * inv_{s,b}) * w'_{s,e}  -- the atomic kernel's expression;
//                  grad_X[v,f] = left-to-right sum of c_e[f] over the entries with col = v, e ascending.
//   embedding bag  entry j = position in the batch's entry order (the dropout key's j), contribution
//                  ((g[m,h] * inv_m) * d_j) * keep_{j,h}*scale;  dW[a,h] = left-to-right sum over a_j = a, j ascending.
// -ffp-contract=off applies as in the other units: no product is fused into the add that follows it.
//
// Mapping.  A wave takes a window of 64 consecutive positions of the sorted list.  Its lanes read their own position's
// key and ballot the head flags key[i] != key[i-1]; each lane also prepares its own position's entry (the weights and
// denominators of the rows form, (m, j, d_j, inv_m) of the bag: the hash and the dependent loads run 64 entries at a
// time).  Then, per head in the window, the 64 lanes cover 64 consecutive floats of the destination row (kCols of
// them per pass for wider rows) and walk the segment to its end: first through the window's prepared entries, passed
// round with shuffles, then, when the segment runs past the window, through further groups of 64 prepared the same
// way.  A position whose key is not a destination (the sentinel N / V, to which the caller keys what does not exist)
// ends the walk.  A long segment is a serial chain of adds on one wave: the accepted cost of the mode (§7i); the two
// _chunked entry points at the end of this unit cut it into chunks (§7w, gather_chunk.hpp).
//
// The entry must be found exactly as the forward finds it: BagLayout, bag_of, attr_id, sample_weight and the
// denominators are dropnode.hpp's, the lines augment.hip calls.
#include "dropnode.hpp"
#include "gather_sum.hpp"
#include "gather_chunk.hpp"
#include "gather_chunk_abi.hpp"

#include <algorithm>

namespace {

constexpr int kBlock = 256;           // the pre-pass kernels
constexpr int kDenSamples = 4;        // samples whose weights the rows pre-pass stages at a time

// ---- pre-pass, rows form: inv_den[s * n_batch + b] = 1 / (den_{s,b} + 1e-12), den summed over k in the forward's order
__global__ void __launch_bounds__(kBlock)
rows_inv_den_kernel(const double* __restrict__ val, const int* __restrict__ filled, int K, const int* __restrict__ batch_rows,
                    int n_batch, int S, float p, int training, u64 seed, const unsigned char* __restrict__ keep,
                    long long keep_stride, float* __restrict__ inv_den)
{
    __shared__ float s_w[kDenSamples][kStage];
    const float scale = inv_keep(p);
    for (int b = blockIdx.x; b < n_batch; b += gridDim.x) {
        const long long row = batch_rows ? batch_rows[b] : b;
        const int n = row_len(filled, row, K);
        for (int s0 = 0; s0 < S; s0 += kDenSamples) {
            const int ns = min(kDenSamples, S - s0);
            __syncthreads();
            for (int k = threadIdx.x; k < n; k += kBlock) {
                const long long e = row * (long long)K + k;
                const float w = (float)val[e];
                for (int s = 0; s < ns; ++s) s_w[s][k] = sample_weight(w, e, s0 + s, p, scale, training, seed, keep, keep_stride);
            }
            __syncthreads();
            if (threadIdx.x < ns) {
                float den = 0.0f;
                for (int k = 0; k < n; ++k) den += s_w[threadIdx.x][k];
                inv_den[(size_t)(s0 + threadIdx.x) * n_batch + b] = inv_den_rows(den);
            }
        }
    }
}

// ---- pre-pass, embedding bag: inv_den[m] = 1 / (den_m + 1e-10), den summed as embedding_bag_backward_kernel sums it;
// bag sources outside [0, n_src) and ids outside [0, V) are counted as that kernel counts them.
__global__ void __launch_bounds__(kBlock)
bag_inv_den_kernel(long long V, BagLayout L, float* __restrict__ inv_den, int* __restrict__ n_bad)
{
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * kBlock + threadIdx.x) >> 6;
    const long long n_waves = ((long long)gridDim.x * kBlock) >> 6;
    for (long long m = wave; m < L.n_rows; m += n_waves) {        // wave-uniform loop
        long long s0, s1, jb;
        if (!bag_of(L, m, s0, s1, jb)) {
            if (lane == 0) { inv_den[m] = 0.0f; if (n_bad) atomicAdd(n_bad, 1); }
            continue;
        }
        float den = 0.0f;
        for (long long c0 = s0; c0 < s1; c0 += 64) {
            const bool cl = c0 + lane < s1;
            float part = cl ? L.data[c0 + lane] : 0.0f;
            if (cl && n_bad) { const long long a = attr_id(L, c0 + lane); if (a < 0 || a >= V) atomicAdd(n_bad, 1); }
            for (int o = 1; o < 64; o <<= 1) part += __shfl_xor(part, o);
            den += part;
        }
        if (lane == 0) inv_den[m] = inv_den_bag(den);
    }
}

// ---- what one sorted position contributes.  load(): every lane prepares the entry of its own position i (key: the
// position's sorted key; want: the lane has one); an entry that is not there, or whose key is not its destination,
// comes back dead and adds nothing.  add(): the whole wave adds the entry lane u holds to acc, lane's columns
// f + 64*c (c < kCols) of the destination row.
struct RowsOp {
    const float* g; int F; const int* col; const double* val; const int* filled; int K; const int* batch_rows; int n_batch;
    int S; float p; int training; u64 seed; const unsigned char* keep; long long keep_stride; const float* inv_den;

    struct Entry { int b; int live; float w[kMaxSamples], inv[kMaxSamples]; };

    __device__ __forceinline__ Entry load(const long long* __restrict__ order, long long i, bool want, long long key) const
    {
        Entry E;
        E.b = 0; E.live = 0;
#pragma unroll
        for (int s = 0; s < kMaxSamples; ++s) E.w[s] = E.inv[s] = 0.0f;
        if (!want) return E;
        const long long e = order[i];
        if (e < 0 || e >= (long long)n_batch * K) return E;
        const int b = (int)(e / K), k = (int)(e - (long long)b * K);
        const long long row = batch_rows ? batch_rows[b] : b;
        const int n = row_len(filled, row, K);
        const long long re = row * (long long)K + k;              // the resident slot: keys the mask, as in the forward
        if (k >= n || (long long)col[re] != key) return E;
        const float scale = inv_keep(p);
        const float w = (float)val[re];
        bool any = false;
#pragma unroll
        for (int s = 0; s < kMaxSamples; ++s) {
            if (s < S) {
                E.w[s] = sample_weight(w, re, s, p, scale, training, seed, keep, keep_stride);
                E.inv[s] = inv_den[(size_t)s * n_batch + b];
                any |= E.w[s] != 0.0f;
            }
        }
        E.b = b; E.live = any;                                       // dropped in every sample: adds nothing, g is not read
        return E;
    }

    __device__ __forceinline__ void add(const Entry& E, int u, int f, float (&acc)[kCols]) const
    {
        if (!__shfl(E.live, u)) return;                              // wave-uniform
        const float* gb = g + (size_t)__shfl(E.b, u) * F;
        const size_t g_stride = (size_t)n_batch * F;
        float x[kCols];
#pragma unroll
        for (int c = 0; c < kCols; ++c) x[c] = 0.0f;
#pragma unroll
        for (int s = 0; s < kMaxSamples; ++s) {
            if (s < S) {
                const float inv = __shfl(E.inv[s], u), w = __shfl(E.w[s], u);
#pragma unroll
                for (int c = 0; c < kCols; ++c)
                    if (f + 64 * c < F) x[c] += (gb[s * g_stride + f + 64 * c] * inv) * w;
            }
        }
#pragma unroll
        for (int c = 0; c < kCols; ++c) acc[c] += x[c];
    }
};

struct BagOp {
    const float* g; int H; BagLayout L; float p; int training; u64 seed; const unsigned char* keep; const float* inv_den;
    const long long* rows;                                           // [n_sorted]: the output row m of each sorted position

    struct Entry { long long m, j; float d, inv; int live; };

    __device__ __forceinline__ Entry load(const long long* __restrict__ order, long long i, bool want, long long key) const
    {
        Entry E;
        E.m = E.j = 0; E.d = E.inv = 0.0f; E.live = 0;
        if (!want) return E;
        const long long j = order[i], m = rows[i];
        long long s0, s1, jb;
        if (m < 0 || m >= L.n_rows || !bag_of(L, m, s0, s1, jb)) return E;
        const long long t = s0 + (j - jb);                           // the entry's storage position
        if (j < jb || t >= s1 || attr_id(L, t) != key) return E;
        E.m = m; E.j = j; E.d = L.data[t]; E.inv = inv_den[m]; E.live = 1;
        return E;
    }

    __device__ __forceinline__ void add(const Entry& E, int u, int f, float (&acc)[kCols]) const
    {
        if (!__shfl(E.live, u)) return;                              // wave-uniform
        const long long m = __shfl(E.m, u), j = __shfl(E.j, u);
        const float d = __shfl(E.d, u), inv = __shfl(E.inv, u);
        const float scale = inv_keep(p);
#pragma unroll
        for (int c = 0; c < kCols; ++c) {
            const int h = f + 64 * c;
            if (h >= H) continue;
            float x = (g[(size_t)m * H + h] * inv) * d;              // embedding_bag_backward_kernel's expression
            if (training) {
                const u64 el = (u64)j * (u64)H + (u64)h;
                x *= keep ? (keep[el] ? scale : 0.0f) : keep_scale(seed, el, p, scale);
            }
            acc[c] += x;
        }
    }
};

// gp_random_prop_rows_backward_det and its chunked twin: the checks, the pre-pass and the Op are the same, the
// gather is gather_sum_kernel, or with a Chunking gather_chunk.hpp's.  where: the entry point that was called.
int rows_backward_det(const char* where, int device, const float* d_grad_out, int32_t n_batch, int32_t feat_dim,
                      const int32_t* d_col, const double* d_val, const int32_t* d_filled, int32_t K, const int32_t* d_batch_rows,
                      int32_t n_samples, float dropnode_rate, int training, uint64_t seed, const uint8_t* d_keep,
                      int64_t keep_stride, float* d_grad_x, int64_t n_nodes, const int64_t* d_order, const int64_t* d_sorted_keys,
                      int64_t n_sorted, float* d_inv_den, const Chunking* chunking, void* stream)
{
    if (n_samples < 1 || n_samples > kMaxSamples || !(dropnode_rate >= 0.0f && dropnode_rate <= 1.0f))
        return fail(GP_ERR_INVALID_ARG, where, "n_samples outside [1, 16] or dropnode_rate outside [0, 1]");
    if (n_batch < 0 || n_nodes < 1 || feat_dim < 1 || K < 1 || K > GP_MAX_K || n_sorted < 0 || (d_keep && keep_stride < 1))
        return fail(GP_ERR_INVALID_ARG, where, "bad size, K outside [1, 1024] or keep_stride < 1 with a mask");
    if (chunking)
        if (const int rc = chunk_check(where, *chunking, n_batch == 0 ? 0 : n_sorted, feat_dim)) return rc;
    if (n_batch == 0 || n_sorted == 0) return GP_OK;
    if (!d_grad_out || !d_col || !d_val || !d_grad_x || !d_order || !d_sorted_keys || !d_inv_den)
        return fail(GP_ERR_NULL, where, "a device pointer is NULL");
    if (const int rc = set_device(device, where)) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(rows_inv_den_kernel, dim3(std::min(n_batch, 65535)), dim3(kBlock), 0, s, d_val, d_filled, K, d_batch_rows,
                       n_batch, n_samples, dropnode_rate, training, (u64)seed, d_keep, (long long)keep_stride, d_inv_den);
    if (const int rc = launch_status("rows_inv_den_kernel")) return rc;
    const RowsOp op = {d_grad_out, feat_dim, d_col, d_val, d_filled, K, d_batch_rows, n_batch, n_samples, dropnode_rate, training,
                       (u64)seed, d_keep, (long long)keep_stride, d_inv_den};
    if (!chunking) {
        hipLaunchKernelGGL(gather_sum_kernel<RowsOp>, dim3(gather_grid(n_sorted)), dim3(kGather), 0, s, op, (const long long*)d_order,
                           (const long long*)d_sorted_keys, (long long)n_sorted, (long long)n_nodes, feat_dim, d_grad_x);
        return launch_status("gather_sum_kernel<RowsOp>");
    }
    return gather_chunked(op, "gather_chunk_kernel<RowsOp>", d_order, d_sorted_keys, n_sorted, n_nodes, feat_dim, chunking->chunk,
                          d_grad_x, chunking->d_scratch, s);
}

}  // namespace

extern "C" {

int gp_random_prop_rows_backward_det(int device, const float* d_grad_out, int32_t n_batch, int32_t feat_dim,
                                     const int32_t* d_col, const double* d_val, const int32_t* d_filled, int32_t K,
                                     const int32_t* d_batch_rows, int32_t n_samples, float dropnode_rate, int training,
                                     uint64_t seed, const uint8_t* d_keep, int64_t keep_stride, float* d_grad_x,
                                     int64_t n_nodes, const int64_t* d_order, const int64_t* d_sorted_keys, int64_t n_sorted,
                                     float* d_inv_den, void* stream)
{
    return rows_backward_det("gp_random_prop_rows_backward_det", device, d_grad_out, n_batch, feat_dim, d_col, d_val, d_filled, K,
                             d_batch_rows, n_samples, dropnode_rate, training, seed, d_keep, keep_stride, d_grad_x, n_nodes, d_order,
                             d_sorted_keys, n_sorted, d_inv_den, nullptr, stream);
}

int gp_embedding_bag_backward_det(int device, const float* d_grad_out, int64_t n_vocab, int32_t dim,
                                  const int64_t* d_offsets, int64_t n_src, const int64_t* d_nodes,
                                  const int64_t* d_entry_base, int64_t n_rows, const void* d_attr_idx, int idx_bytes,
                                  const float* d_attr_data, float dropout_rate, int training, uint64_t seed,
                                  const uint8_t* d_keep, float* d_grad_weight, int32_t* d_n_bad, const int64_t* d_order,
                                  const int64_t* d_sorted_keys, const int64_t* d_sorted_rows, int64_t n_sorted,
                                  float* d_inv_den, void* stream)
{
    const char* where = "gp_embedding_bag_backward_det";
    if (n_vocab < 0 || dim < 1 || n_src < 0 || n_rows < 0 || n_sorted < 0 || (idx_bytes != 4 && idx_bytes != 8) ||
        !(dropout_rate >= 0.0f && dropout_rate <= 1.0f))
        return fail(GP_ERR_INVALID_ARG, where, "negative size, dim < 1, idx_bytes not 4 or 8, or dropout rate outside [0, 1]");
    if (n_rows == 0) return GP_OK;
    if (!d_offsets || !d_attr_idx || !d_attr_data || !d_grad_out || !d_inv_den || (n_vocab > 0 && !d_grad_weight) ||
        (n_sorted > 0 && (!d_order || !d_sorted_keys || !d_sorted_rows)))
        return fail(GP_ERR_NULL, where, "a device pointer is NULL");
    if (const int rc = set_device(device, where)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (d_n_bad && hipMemsetAsync(d_n_bad, 0, sizeof(int32_t), s) != hipSuccess) return fail(GP_ERR_HIP, where, "hipMemsetAsync failed");
    const BagLayout L = bag_layout(d_offsets, n_src, d_nodes, d_entry_base, n_rows, d_attr_idx, idx_bytes, d_attr_data);
    const int grid = (int)std::min<long long>(65535, (n_rows + kBlock / 64 - 1) / (kBlock / 64));
    hipLaunchKernelGGL(bag_inv_den_kernel, dim3(grid), dim3(kBlock), 0, s, (long long)n_vocab, L, d_inv_den, d_n_bad);
    if (const int rc = launch_status("bag_inv_den_kernel")) return rc;
    if (n_sorted == 0 || n_vocab == 0) return GP_OK;
    const BagOp op = {d_grad_out, dim, L, dropout_rate, training, (u64)seed, d_keep, d_inv_den, (const long long*)d_sorted_rows};
    hipLaunchKernelGGL(gather_sum_kernel<BagOp>, dim3(gather_grid(n_sorted)), dim3(kGather), 0, s, op, (const long long*)d_order,
                       (const long long*)d_sorted_keys, (long long)n_sorted, (long long)n_vocab, dim, d_grad_weight);
    return launch_status("gather_sum_kernel<BagOp>");
}

// ---- the chunked twins (gather_chunk_abi.hpp states their contract): the same pre-pass and the same Op, the
// gather cut into chunks of `chunk` sorted positions by gather_chunk.hpp.

int gp_random_prop_rows_backward_det_chunked(int device, const float* d_grad_out, int32_t n_batch, int32_t feat_dim,
                                             const int32_t* d_col, const double* d_val, const int32_t* d_filled, int32_t K,
                                             const int32_t* d_batch_rows, int32_t n_samples, float dropnode_rate, int training,
                                             uint64_t seed, const uint8_t* d_keep, int64_t keep_stride, float* d_grad_x,
                                             int64_t n_nodes, const int64_t* d_order, const int64_t* d_sorted_keys,
                                             int64_t n_sorted, float* d_inv_den, int32_t chunk, float* d_scratch,
                                             int64_t scratch_bytes, void* stream)
{
    const Chunking chunking = {chunk, d_scratch, scratch_bytes};
    return rows_backward_det("gp_random_prop_rows_backward_det_chunked", device, d_grad_out, n_batch, feat_dim, d_col, d_val, d_filled,
                             K, d_batch_rows, n_samples, dropnode_rate, training, seed, d_keep, keep_stride, d_grad_x, n_nodes, d_order,
                             d_sorted_keys, n_sorted, d_inv_den, &chunking, stream);
}

int gp_embedding_bag_backward_det_chunked(int device, const float* d_grad_out, int64_t n_vocab, int32_t dim,
                                          const int64_t* d_offsets, int64_t n_src, const int64_t* d_nodes,
                                          const int64_t* d_entry_base, int64_t n_rows, const void* d_attr_idx, int idx_bytes,
                                          const float* d_attr_data, float dropout_rate, int training, uint64_t seed,
                                          const uint8_t* d_keep, float* d_grad_weight, int32_t* d_n_bad, const int64_t* d_order,
                                          const int64_t* d_sorted_keys, const int64_t* d_sorted_rows, int64_t n_sorted,
                                          float* d_inv_den, int32_t chunk, float* d_scratch, int64_t scratch_bytes, void* stream)
{
    const char* where = "gp_embedding_bag_backward_det_chunked";
    if (n_vocab < 0 || dim < 1 || n_src < 0 || n_rows < 0 || n_sorted < 0 || (idx_bytes != 4 && idx_bytes != 8) ||
        !(dropout_rate >= 0.0f && dropout_rate <= 1.0f))
        return fail(GP_ERR_INVALID_ARG, where, "negative size, dim < 1, idx_bytes not 4 or 8, or dropout rate outside [0, 1]");
    const bool gathers = n_rows > 0 && n_sorted > 0 && n_vocab > 0;
    if (const int rc = chunk_check(where, {chunk, d_scratch, scratch_bytes}, gathers ? n_sorted : 0, dim)) return rc;
    if (gathers && (!d_order || !d_sorted_keys || !d_sorted_rows)) return fail(GP_ERR_NULL, where, "a device pointer is NULL");
    // The pre-pass is the twin's own: given no sorted positions it checks the remaining pointers, counts the bad ids, writes
    // inv_den and stops before its gather.
    if (const int rc = gp_embedding_bag_backward_det(device, d_grad_out, n_vocab, dim, d_offsets, n_src, d_nodes, d_entry_base, n_rows,
                                                     d_attr_idx, idx_bytes, d_attr_data, dropout_rate, training, seed, d_keep,
                                                     d_grad_weight, d_n_bad, nullptr, nullptr, nullptr, 0, d_inv_den, stream))
        return rc;
    if (!gathers) return GP_OK;
    const BagLayout L = bag_layout(d_offsets, n_src, d_nodes, d_entry_base, n_rows, d_attr_idx, idx_bytes, d_attr_data);
    const BagOp op = {d_grad_out, dim, L, dropout_rate, training, (u64)seed, d_keep, d_inv_den, (const long long*)d_sorted_rows};
    return gather_chunked(op, "gather_chunk_kernel<BagOp>", d_order, d_sorted_keys, n_sorted, n_vocab, dim, chunk, d_grad_weight,
                          d_scratch, (hipStream_t)stream);
}

}  // extern "C"
