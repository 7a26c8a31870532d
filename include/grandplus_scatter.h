/*
 * grandplus_scatter.h -- the deterministic scatter backwards of the C ABI (implemented by
 * grand_plus_amd/csrc/scatter_det.hip).
 *
 * Part of the ABI that grandplus.h describes (GP_ABI_VERSION and the status codes are defined there): grandplus.h
 * includes this file, so callers include grandplus.h alone.  The ctypes binding declares these entry points under this
 * file's name in _native.ABI, and tests/test_host_abi.py holds that table against this file type by type.
 */
#ifndef GRANDPLUS_SCATTER_H
#define GRANDPLUS_SCATTER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * gp_random_prop_rows_multi_backward and gp_embedding_bag_backward add into their dense gradient with fp32 atomics, so
 * the sum of a destination row depends on the order in which the adds arrive.  The two entry points here compute the
 * same gradients by sort-then-gather: the caller orders the entries of the call by destination row with a STABLE sort,
 * and one gather kernel sums every destination row that occurs sequentially in that order, from 0.0f, and writes it
 * once with plain stores.  No atomics touch the gradient: it is bitwise the same run to run.  Rows that do not occur
 * keep the caller's zeros (d_grad_x / d_grad_weight are caller-zeroed, as for the atomic entry points).
 *
 * The sorted order is three device arrays of n_sorted entries:
 *   d_order        int64  the entry numbers, ordered by destination and, within one destination, ascending;
 *   d_sorted_keys  int64  the destination row of d_order[i]: ascending.  A key outside [0, n_nodes) / [0, n_vocab)
 *                         marks an entry that does not exist or is skipped; the caller keys such entries to the sentinel
 *                         n_nodes / n_vocab, so that they sort last and end the walk of the last segment;
 *   (embedding bag) d_sorted_rows int64  the output row m of d_order[i].
 * An entry number, row or storage position outside its array is never used as an address: the entry adds nothing.
 *
 * Order contract, rows form (gp_random_prop_rows_backward_det; n_samples = 1 is the single-sample backward, with
 * d_grad_out [n_batch x feat_dim]):
 *   entry e = b * K + k, b the position in the batch (not the resident row r = d_batch_rows[b]), k < min(filled[r], K);
 *   its contribution to d_grad_x[col[r,k], f] is
 *       c_e[f] = sum over s = 0 .. n_samples-1, in that order, from 0.0f, of (g[s,b,f] * inv_{s,b}) * w'_{s,e}
 *   with w'_{s,e} the forward's weight (mask from gp_sample_seed(seed, s) or d_keep[s * keep_stride + r*K + k]) and
 *   inv_{s,b} = 1 / (den_{s,b} + 1e-12), den the forward's sequential sum over k: the expression of
 *   gp_random_prop_rows_multi_backward.  An entry whose weight is 0 in every sample adds nothing and its g is not read.
 *   d_grad_x[v, f] = the left-to-right sum of c_e[f] over the entries with col = v, e ascending.  A batch that names a
 *   resident row twice contributes it twice.  Column ids outside [0, n_nodes) are skipped; unfilled slots do not exist.
 *
 * Order contract, embedding bag (gp_embedding_bag_backward_det):
 *   entry j = the entry's position in the batch's entry order (d_entry_base[m] + t, or the storage position), the j that
 *   keys the dropout of element (j, h) as j * dim + h;
 *   its contribution to d_grad_weight[a_j, h] is ((g[m,h] * inv_m) * d_j) * keep_{j,h}*scale, inv_m = 1 / (den_m + 1e-10)
 *   with den_m summed as gp_embedding_bag_backward sums it (64 entries at a time, a wave butterfly per 64);
 *   d_grad_weight[a, h] = the left-to-right sum over the entries with a_j = a, j ascending.
 *   Ids outside [0, n_vocab) and bag sources outside [0, n_src) are never read or written; they are counted into
 *   d_n_bad (NULL: not counted) exactly as gp_embedding_bag_backward counts them.
 *
 * d_inv_den is the caller's scratch: GP_SCATTER_ROWS_WORKSPACE_BYTES(n_samples, n_batch) /
 * GP_SCATTER_BAG_WORKSPACE_BYTES(n_rows) bytes of device memory, 4-byte aligned; a small pre-pass kernel fills it with
 * the inv_{s,b} / inv_m above before the gather kernel runs.
 *
 * Contracts: arguments are checked before the device is touched (GP_ERR_INVALID_ARG for a negative size, K outside
 * [1, 1024], n_samples outside [1, 16], a rate outside [0, 1], idx_bytes not 4 or 8; GP_ERR_NULL for a missing pointer);
 * an empty call (n_batch = 0 / n_rows = 0 / n_sorted = 0) returns GP_OK without a launch; both enqueue on `stream`;
 * nothing on the call path allocates, copies to the host or synchronises.
 * ------------------------------------------------------------------------------------------ */
#define GP_SCATTER_ROWS_WORKSPACE_BYTES(n_samples, n_batch) (4 * (int64_t)(n_samples) * (int64_t)(n_batch))
#define GP_SCATTER_BAG_WORKSPACE_BYTES(n_rows) (4 * (int64_t)(n_rows))

int gp_random_prop_rows_backward_det(int device, const float* d_grad_out, int32_t n_batch, int32_t feat_dim,
                                     const int32_t* d_col, const double* d_val, const int32_t* d_filled, int32_t K,
                                     const int32_t* d_batch_rows, int32_t n_samples, float dropnode_rate, int training,
                                     uint64_t seed, const uint8_t* d_keep, int64_t keep_stride, float* d_grad_x,
                                     int64_t n_nodes, const int64_t* d_order, const int64_t* d_sorted_keys, int64_t n_sorted,
                                     float* d_inv_den, void* stream);
int gp_embedding_bag_backward_det(int device, const float* d_grad_out, int64_t n_vocab, int32_t dim,
                                  const int64_t* d_offsets, int64_t n_src, const int64_t* d_nodes,
                                  const int64_t* d_entry_base, int64_t n_rows, const void* d_attr_idx, int idx_bytes,
                                  const float* d_attr_data, float dropout_rate, int training, uint64_t seed,
                                  const uint8_t* d_keep, float* d_grad_weight, int32_t* d_n_bad, const int64_t* d_order,
                                  const int64_t* d_sorted_keys, const int64_t* d_sorted_rows, int64_t n_sorted,
                                  float* d_inv_den, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GRANDPLUS_SCATTER_H */
