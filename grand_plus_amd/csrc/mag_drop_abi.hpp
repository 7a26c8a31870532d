/*
 * mag_drop_abi.hpp -- MAG's front end with the seed in device memory, and its deterministic table gradient with input
 * dropout (implemented by csrc/mag_prop.hip and csrc/mag_drop.hip).
 *
 * NOT part of C ABI 4: these are extern "C" symbols of libgrandplus.so that no public header declares.  The callers are
 * grand_plus_amd/mag.py and grand_plus_amd/mag_drop.py; _native.PRIVATE_ABI binds them, under this file's name and the
 * convention of _native.ABI: d_* and void* travel as c_void_p, scalars map one to one.  tests/test_host_abi.py holds that
 * table against this file.
 *
 * The device seed.  d_seed points to one uint64 in device memory.  Every kernel of a call reads it once, before its row
 * loop, and derives from that value what the value forms derive from `seed`: the hashed DropNode mask and
 * GP_MAG_SLOT_SEED (grandplus_mag.h).  A captured graph freezes the pointer, not the value: a replay draws the masks of
 * the value that stands there when it runs.  Nothing else changes: same kernels, same order contract, same bounds rules,
 * same checks, and with the value v behind d_seed the result is bit for bit the value form's with seed = v (the backward's
 * up to the order of its atomics).
 *
 * The deterministic backward with input dropout.  Slots, entries, keys, d_slot_base, the caller's stable sort and the
 * overflow flag are gp_mag_det_keys' (mag_det_abi.hpp) and unchanged.  With input dropout every (sample s, bag position t,
 * column h) has its own mask factor, so the slot gradient is kept per sample:
 *
 * Order contract.  For slot e = b * K + k of resident row r = d_batch_rows[b], n its node:
 *     U[s, e, h]  = ((g[s, b, h] * inv_{s,b}) * w'_{s,k}) * inv_den_n              0 where w'_{s,k} == 0
 *     x_j[h]      = sum over s ascending, from 0.0f, samples with w'_{s,k} == 0 passed over, of
 *                   (U[s, e_j, h] * d_j) * m_in(s, r * K + k, t, h)
 *     dW[a, h]    = the left-to-right fp32 sum, from 0.0f, of x_j[h] over the entries with a_j = a, j ascending
 * where w', inv_{s,b} = 1 / (sum_k w'_{s,k} + 1e-12) and inv_den_n = 1 / (sum_t d_t + 1e-10) are the forward's, both sums
 * taken sequentially in the forward's order: these are the atomic backward's own expressions (grandplus_mag.h).
 * m_in(s, r * K + k, t, h) = keep_scale(GP_MAG_SLOT_SEED(seed, s, r * K + k), t * dim + h, input_droprate,
 * 1 / (1 - input_droprate)) is grandplus_mag.h's: the slot of the seed is the RESIDENT slot r * K + k, not the batch slot
 * e, and t is the entry's position in its node's bag.  When no mask is drawn (eval mode, or input_droprate = 0) m_in is 1.
 * No product is fused into the add that follows it (-ffp-contract=off).  Rows of dW that no entry names keep the caller's
 * values: the caller passes zeros.  The result is bitwise the same from run to run.
 * With chunk != 0 the x_j of a destination are summed by the contract of gather_chunk_abi.hpp (chunks counted from the
 * segment's first sorted position, folded in chunk order); a destination of at most `chunk` entries gets the bits of
 * chunk = 0.
 *
 * Common contract: arguments are checked before the device is touched; nothing on a call path reads a device value on the
 * host, allocates, copies or synchronises, so every launch can be captured; gp_mag_prop_rows_backward_det_drop uses no
 * atomics; all offsets are 64-bit.
 */
#pragma once

#include <stdint.h>

#include "grandplus.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gp_mag_prop_rows (grandplus_mag.h) with the seed read from *d_seed.  GP_ERR_NULL also for d_seed = NULL (with n_batch > 0). */
int gp_mag_prop_rows_dseed(int device, const float* d_weight, int64_t n_vocab, int32_t dim, const int64_t* d_attr_indptr,
                           const int32_t* d_attr_indices, const float* d_attr_data, int64_t n_nodes, const int32_t* d_col,
                           const double* d_val, const int32_t* d_filled, int64_t n_rows, int32_t K,
                           const int32_t* d_batch_rows, int32_t n_batch, int32_t n_samples, float dropnode_rate,
                           float input_droprate, int training, const uint64_t* d_seed, const uint8_t* d_keep,
                           int64_t keep_stride, float* d_out, int32_t* d_n_bad, void* stream);

/* gp_mag_prop_rows_backward (grandplus_mag.h) with the seed read from *d_seed.  GP_ERR_NULL also for d_seed = NULL. */
int gp_mag_prop_rows_backward_dseed(int device, const float* d_grad_out, int64_t n_vocab, int32_t dim,
                                    const int64_t* d_attr_indptr, const int32_t* d_attr_indices, const float* d_attr_data,
                                    int64_t n_nodes, const int32_t* d_col, const double* d_val, const int32_t* d_filled,
                                    int64_t n_rows, int32_t K, const int32_t* d_batch_rows, int32_t n_batch,
                                    int32_t n_samples, float dropnode_rate, float input_droprate, int training,
                                    const uint64_t* d_seed, const uint8_t* d_keep, int64_t keep_stride, float* d_dW,
                                    void* stream);

/* ------------------------------------------------------------------------------------------
 * dW by the order contract above.  The arguments of gp_mag_prop_rows_backward_det (mag_det_abi.hpp), with d_seed after
 * seed (NULL: the value `seed`) and chunk, d_scratch, scratch_bytes before the stream.  d_slot_grad is float
 * [n_samples * n_batch * K * dim]: U[s, e, :] at ((s * n_batch * K) + e) * dim; d_inv float [n_samples * n_batch].
 * chunk = 0: the unchunked gather, d_scratch and scratch_bytes are not looked at.  Any other chunk must be a power of two
 * in [64, 4096] with a scratch of GP_GATHER_CHUNK_SCRATCH_BYTES(max_entries, chunk, dim) (gather_chunk_abi.hpp):
 * GP_ERR_INVALID_ARG for another chunk or a smaller scratch, GP_ERR_NULL for a NULL d_scratch where bytes are needed.
 * Two launches, three with a chunk: U and inv, then the gather (and the fold).
 * Otherwise the checks are gp_mag_prop_rows_backward_det's, input dropout accepted: GP_ERR_INVALID_ARG for a bad size
 * or rate, max_entries < 1 or n_batch * K >= 2^31; GP_ERR_NULL for a missing pointer.  n_batch = 0 is GP_OK with nothing
 * launched.
 * ------------------------------------------------------------------------------------------ */
int gp_mag_prop_rows_backward_det_drop(int device, const float* d_grad_out, int64_t n_vocab, int32_t dim,
                                       const int64_t* d_attr_indptr, const int32_t* d_attr_indices, const float* d_attr_data,
                                       int64_t n_nodes, const int32_t* d_col, const double* d_val, const int32_t* d_filled,
                                       int64_t n_rows, int32_t K, const int32_t* d_batch_rows, int32_t n_batch,
                                       int32_t n_samples, float dropnode_rate, float input_droprate, int training,
                                       uint64_t seed, const uint64_t* d_seed, const uint8_t* d_keep, int64_t keep_stride,
                                       const int64_t* d_slot_base, const int64_t* d_order, const int64_t* d_sorted_keys,
                                       int64_t max_entries, float* d_slot_grad, float* d_inv, float* d_dW, int32_t chunk,
                                       float* d_scratch, int64_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
