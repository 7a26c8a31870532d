/*
 * gather_chunk_abi.hpp -- the entry points of the chunked deterministic gradients (implemented by
 * csrc/scatter_det.hip and csrc/mag_det.hip over the kernels of csrc/gather_chunk.hpp).
 *
 * NOT part of C ABI 4: these are extern "C" symbols of libgrandplus.so that no public header declares.  The callers are
 * the three deterministic backwards (augment.py, embedding.py, mag_det.py, with gather_chunk.py's scratch);
 * _native.PRIVATE_ABI binds them, under this file's name and the convention of _native.ABI: d_* and void* travel as
 * c_void_p, scalars map one to one.  tests/test_host_abi.py holds that table against this file.
 *
 * Each is its unchunked twin (gp_random_prop_rows_backward_det and gp_embedding_bag_backward_det of grandplus_scatter.h,
 * gp_mag_prop_rows_backward_det of mag_det_abi.hpp) with three more arguments before the stream: chunk, d_scratch and
 * scratch_bytes.  Operands, bounds rules, pre-passes and what one sorted position contributes are the twin's.  What
 * changes is the order in which a destination's contributions are summed.
 *
 * Order contract.  Take a destination a whose segment occupies the sorted positions q0 .. q0 + n - 1 of the stably sorted
 * key list, and let x_i be what position q0 + i contributes by the twin's contract (a position whose entry fails the
 * twin's re-check contributes nothing, but still counts as a position).  With C = chunk and P = ceil(n / C),
 *     partial_p = the left-to-right fp32 sum, from 0.0f, of x_{pC} .. x_{min((p+1)C, n) - 1}        p = 0 .. P - 1
 *     dst[a]    = the left-to-right fp32 sum, from 0.0f, of partial_0 .. partial_{P-1}.
 * Chunks are counted from the segment's own first position q0, not from window, span or grid boundaries: the bits do not
 * depend on where the segment falls in the list.  No product is fused into the add that follows it (-ffp-contract=off).
 * For n <= C this is bit for bit the twin's contract: P = 1, and a sum that starts at +0.0f is never -0.0f, so
 * 0.0f + partial_0 == partial_0.  The serial chain of a destination is at most C adds plus P adds, whatever n is.
 *
 * chunk is a power of two in [64, 4096]; anything else is GP_ERR_INVALID_ARG.
 *
 * The scratch is the caller's: float rows of the destination's width, GP_GATHER_CHUNK_SCRATCH_BYTES(n_sorted, chunk, width)
 * bytes, a function of those three numbers alone (n_sorted is max_entries in the MAG form).  It need not be initialised and
 * holds nothing afterwards.  A scratch_bytes below that figure is GP_ERR_INVALID_ARG; a NULL d_scratch where bytes are
 * needed is GP_ERR_NULL.  Every scratch index is derived from a sorted position, never from a key alone, so it is in range
 * for any key array, sorted or not; a key outside [0, n_dest) is never a destination.
 *
 * Common contract: arguments are checked before the device is touched; nothing on a call path reads a device value on the
 * host, allocates, copies or synchronises, so every launch can be captured; no atomics on floats, plain stores only; all
 * offsets are 64-bit.  Three launches each: the twin's pre-pass, gather_chunk_kernel, gather_fold_kernel.
 */
#pragma once

#include <stdint.h>

#include "grandplus.h"

/* Two rows per span of `chunk` sorted positions (csrc/gather_chunk_layout.hpp says why two suffice). */
#define GP_GATHER_CHUNK_SCRATCH_BYTES(n_sorted, chunk, width) \
    ((int64_t)2 * (((int64_t)(n_sorted) + (int64_t)(chunk) - 1) / (int64_t)(chunk)) * (int64_t)(width) * 4)

#ifdef __cplusplus
extern "C" {
#endif

/* gp_random_prop_rows_backward_det by the contract above; width = feat_dim. */
int gp_random_prop_rows_backward_det_chunked(int device, const float* d_grad_out, int32_t n_batch, int32_t feat_dim,
                                             const int32_t* d_col, const double* d_val, const int32_t* d_filled, int32_t K,
                                             const int32_t* d_batch_rows, int32_t n_samples, float dropnode_rate, int training,
                                             uint64_t seed, const uint8_t* d_keep, int64_t keep_stride, float* d_grad_x,
                                             int64_t n_nodes, const int64_t* d_order, const int64_t* d_sorted_keys,
                                             int64_t n_sorted, float* d_inv_den, int32_t chunk, float* d_scratch,
                                             int64_t scratch_bytes, void* stream);

/* gp_embedding_bag_backward_det by the contract above; width = dim. */
int gp_embedding_bag_backward_det_chunked(int device, const float* d_grad_out, int64_t n_vocab, int32_t dim,
                                          const int64_t* d_offsets, int64_t n_src, const int64_t* d_nodes,
                                          const int64_t* d_entry_base, int64_t n_rows, const void* d_attr_idx, int idx_bytes,
                                          const float* d_attr_data, float dropout_rate, int training, uint64_t seed,
                                          const uint8_t* d_keep, float* d_grad_weight, int32_t* d_n_bad, const int64_t* d_order,
                                          const int64_t* d_sorted_keys, const int64_t* d_sorted_rows, int64_t n_sorted,
                                          float* d_inv_den, int32_t chunk, float* d_scratch, int64_t scratch_bytes, void* stream);

/* gp_mag_prop_rows_backward_det by the contract above; width = dim, n_sorted = max_entries.  Input dropout stays refused. */
int gp_mag_prop_rows_backward_det_chunked(int device, const float* d_grad_out, int64_t n_vocab, int32_t dim,
                                          const int64_t* d_attr_indptr, const int32_t* d_attr_indices, const float* d_attr_data,
                                          int64_t n_nodes, const int32_t* d_col, const double* d_val, const int32_t* d_filled,
                                          int64_t n_rows, int32_t K, const int32_t* d_batch_rows, int32_t n_batch,
                                          int32_t n_samples, float dropnode_rate, float input_droprate, int training,
                                          uint64_t seed, const uint8_t* d_keep, int64_t keep_stride, const int64_t* d_slot_base,
                                          const int64_t* d_order, const int64_t* d_sorted_keys, int64_t max_entries,
                                          float* d_slot_grad, float* d_inv, float* d_dW, int32_t chunk, float* d_scratch,
                                          int64_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
