/*
 * mag_det_abi.hpp -- the entry points of MAG's deterministic table gradient (implemented by csrc/mag_det.hip).
 *
 * NOT part of C ABI 4: these are extern "C" symbols of libgrandplus.so that no public header declares.  The one caller
 * is grand_plus_amd/mag_det.py; _native.PRIVATE_ABI binds them, under this file's name and the convention of _native.ABI:
 * d_* and void* travel as c_void_p, scalars map one to one.  tests/test_host_abi.py holds that table against this file.
 * Promoting them to a public header is a later change.
 *
 * They are the backward of gp_mag_prop_rows (grandplus_mag.h) without atomics on dW: sort-then-gather, as
 * grandplus_scatter.h's two.  The operands named as in grandplus_mag.h mean what they mean there, and the bounds rules are
 * the same: a batch row outside [0, n_rows), a column outside [0, n_nodes) and an attribute id outside [0, n_vocab) are
 * never used as an address and contribute nothing.
 *
 * Slots and entries.  A slot is e = b * K + k, b the position in the batch, k < K.  It EXISTS when
 * r = d_batch_rows[b] (b without d_batch_rows) lies in [0, n_rows), k < min(d_filled[r], K) (K without d_filled) and
 * d_col[r * K + k] lies in [0, n_nodes).  len_e = the bag length of its node for a slot that exists, 0 for every other.
 * Entry j = base_e + t, base the exclusive prefix sum of len over e, t < len_e: the entries in the order (b, k, t).  Entry
 * j has the attribute id a_j and the weight d_j of position t of its node's bag.
 *
 * Order contract.  With
 *     c_e[h] = sum_s (g[s, b, h] * inv_{s,b}) * w'_{s,k}       s ascending, from 0.0f
 *     U[e, h] = c_e[h] * inv_den_n                              n the slot's node
 * where w', inv_{s,b} = 1 / (sum_k w'_{s,k} + 1e-12) and inv_den_n = 1 / (sum_t d_t + 1e-10) are the forward's, both sums
 * taken sequentially in the forward's order (grandplus_mag.h; they are the atomic backward's own expressions),
 *     dW[a, h] = the left-to-right fp32 sum, from 0.0f, of U[e_j, h] * d_j over the entries with a_j = a, j ascending.
 * No product is fused into the add that follows it (-ffp-contract=off).  A slot dropped in every sample has U = 0 and adds
 * zeros.  Rows of dW that no entry names keep the caller's values: the caller passes zeros.  A batch that names a resident
 * row twice contributes it twice.  The result is bitwise the same from run to run.
 *
 * Common contract: arguments are checked before the device is touched; nothing on a call path reads a device value on the
 * host, allocates, copies or synchronises, so every launch can be captured; no atomics; all offsets are 64-bit.
 * n_batch * K must stay below 2^31.
 */
#pragma once

#include <stdint.h>

#include "grandplus.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * The keys of the call's entries, for the caller's stable sort.  Three launches on `stream`:
 *   1. len_e of every slot;
 *   2. d_slot_base (int64 [n_batch * K + 1]) = the exclusive prefix sum of len; its last element is the total;
 *   3. d_keys (int64 [max_entries]): d_keys[j] = a_j for an id in [0, n_vocab), n_vocab (the sentinel, which is never a
 *      destination) for an id out of range and for the tail [min(total, max_entries), max_entries).
 * An entry with j >= max_entries is written nowhere; if there is one, bit 0 of *d_flag (int32) is set with a plain store
 * (never cleared here), and the gradient that gp_mag_prop_rows_backward_det then gives lacks those entries.
 * GP_ERR_INVALID_ARG: n_vocab < 1, a negative size, K outside [1, 1024], max_entries < 1 or n_batch * K >= 2^31.
 * GP_ERR_NULL: a pointer other than d_filled and d_batch_rows missing.  n_batch = 0 is GP_OK with nothing launched.
 * ------------------------------------------------------------------------------------------ */
int gp_mag_det_keys(int device, int64_t n_vocab, const int64_t* d_attr_indptr, const int32_t* d_attr_indices, int64_t n_nodes,
                    const int32_t* d_col, const int32_t* d_filled, int64_t n_rows, int32_t K, const int32_t* d_batch_rows,
                    int32_t n_batch, int64_t max_entries, int64_t* d_slot_base, int64_t* d_keys, int32_t* d_flag, void* stream);

/* ------------------------------------------------------------------------------------------
 * dW by the order contract above.  The arguments of gp_mag_prop_rows_backward up to keep_stride, then d_slot_base as
 * gp_mag_det_keys wrote it, d_order (the entry number j of every sorted position) and d_sorted_keys (int64 [max_entries]
 * each: the caller's STABLE sort of d_keys), max_entries, the scratch d_slot_grad (float [n_batch * K * dim], U) and d_inv
 * (float [n_samples * n_batch], inv_{s,b}), and d_dW (float [n_vocab, dim], zeroed by the caller).  Two launches: U and
 * inv, then the gather.  The gather finds every entry again from d_slot_base and the call's operands, as the forward found
 * it; a sorted position whose entry does not exist, lies at or past min(total, max_entries), or whose id is not its key
 * adds nothing.
 * Input dropout is not supported here: training with input_droprate > 0 is GP_ERR_INVALID_ARG.  The entry point that takes it
 * is gp_mag_prop_rows_backward_det_drop (mag_drop_abi.hpp), which keeps U per sample.  Otherwise the
 * checks are gp_mag_prop_rows_backward's, plus max_entries < 1 and n_batch * K >= 2^31 (GP_ERR_INVALID_ARG) and the
 * added pointers (GP_ERR_NULL).  n_batch = 0 is GP_OK with nothing launched.
 * ------------------------------------------------------------------------------------------ */
int gp_mag_prop_rows_backward_det(int device, const float* d_grad_out, int64_t n_vocab, int32_t dim,
                                  const int64_t* d_attr_indptr, const int32_t* d_attr_indices, const float* d_attr_data,
                                  int64_t n_nodes, const int32_t* d_col, const double* d_val, const int32_t* d_filled,
                                  int64_t n_rows, int32_t K, const int32_t* d_batch_rows, int32_t n_batch,
                                  int32_t n_samples, float dropnode_rate, float input_droprate, int training,
                                  uint64_t seed, const uint8_t* d_keep, int64_t keep_stride, const int64_t* d_slot_base,
                                  const int64_t* d_order, const int64_t* d_sorted_keys, int64_t max_entries,
                                  float* d_slot_grad, float* d_inv, float* d_dW, void* stream);

#ifdef __cplusplus
}
#endif
