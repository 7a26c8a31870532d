/*
 * row_mark_abi.hpp -- the entry points that give MAG's atomic table gradient a row list (implemented by
 * csrc/row_mark.hip).
 *
 * NOT part of C ABI 4: these are extern "C" symbols of libgrandplus.so that no public header declares, as
 * mag_det_abi.hpp's and optim_rows_abi.hpp's.  The one caller is grand_plus_amd/optim_rows.py; _native.PRIVATE_ABI binds
 * them, under this file's name and the convention of _native.ABI: d_* and void* travel as c_void_p, scalars map one to
 * one.  tests/test_host_abi.py holds that table against this file.
 *
 * The atomic backward (gp_mag_prop_rows_backward, grandplus_mag.h) adds into a dense dW and keeps no list of the rows it
 * added into.  Here the rows a batch CAN touch are marked in a bitmap of n_vocab bits (csrc/row_mark_layout.hpp states
 * the layout), the bitmap is compacted into the list that optim_rows_abi.hpp consumes -- int64 keys, ascending, each row
 * once, the sentinel n_vocab in the tail -- and the listed rows of dW are zeroed, so that dW need not be zero-filled and
 * is read on listed rows alone.  The list is the same from run to run although the marking is atomic: an OR is
 * idempotent and commutative.
 *
 * d_bitmap is int32 [(n_vocab + 31) / 32], all zero before gp_row_mark_mag; gp_row_list_compact leaves it all zero again.
 *
 * Common contract: arguments are checked before the device is touched; nothing on a call path reads a device value on the
 * host, allocates, copies or synchronises, so every launch can be captured; all offsets are 64-bit.
 */
#pragma once

#include <stdint.h>

#include "grandplus.h"

#define GP_ROW_LIST_PARTIALS 1024   /* int64 elements of gp_row_list_compact's d_partials */

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Marks the rows of the table that the batch's bags name.  One launch on `stream`.  The operands named as in
 * mag_det_abi.hpp mean what they mean there; a slot e = b * K + k EXISTS by the rule stated there.  For every slot that
 * exists and every attribute id a of its node's bag with 0 <= a < n_vocab, bit a of d_bitmap is set with an atomic OR.
 * Every existing slot is marked, whether or not DropNode kept it: the marked set is the set of distinct in-range keys that
 * gp_mag_det_keys writes with an unbounded max_entries, a superset of the rows gp_mag_prop_rows_backward adds into.  A
 * batch row outside [0, n_rows), a column outside [0, n_nodes) and an attribute id outside [0, n_vocab) are never used as
 * an address and mark nothing.
 * GP_ERR_INVALID_ARG: n_vocab < 1, a negative size, K outside [1, 1024] or n_batch * K >= 2^31.  GP_ERR_NULL: a pointer
 * other than d_filled and d_batch_rows missing.  n_batch = 0 is GP_OK with nothing launched.
 * ------------------------------------------------------------------------------------------ */
int gp_row_mark_mag(int device, int64_t n_vocab, const int64_t* d_attr_indptr, const int32_t* d_attr_indices, int64_t n_nodes,
                    const int32_t* d_col, const int32_t* d_filled, int64_t n_rows, int32_t K, const int32_t* d_batch_rows,
                    int32_t n_batch, int32_t* d_bitmap, void* stream);

/* ------------------------------------------------------------------------------------------
 * The list of the marked rows.  Two launches on `stream` over the same grid of at most 1 024 workgroups, each of which
 * owns a contiguous chunk of the bitmap's words:
 *   1. d_partials[g] (int64 [GP_ROW_LIST_PARTIALS]) = the number of set bits below n_vocab in chunk g;
 *   2. every workgroup adds the partials before its own in a fixed order, scans its chunk and writes row r to
 *      d_keys[pos_r] (int64 [capacity]), pos_r the number of marked rows below r, while pos_r < capacity; stores 0 to
 *      every word of its chunk; fills d_keys[min(total, capacity) .. capacity) with n_vocab; *d_count (int64) = total,
 *      unclamped.  If total > capacity, bit 0 of *d_flag (int32) is set with a plain store (never cleared here) and the
 *      list holds the first `capacity` marked rows.
 * No atomics.  A bit at or above n_vocab is neither counted nor listed, and is cleared like every other.
 * GP_ERR_INVALID_ARG: n_vocab < 1 or capacity < 1.  GP_ERR_NULL: a pointer missing.
 * ------------------------------------------------------------------------------------------ */
int gp_row_list_compact(int device, int64_t n_vocab, int32_t* d_bitmap, int64_t capacity, int64_t* d_keys, int64_t* d_count,
                        int64_t* d_partials, int32_t* d_flag, void* stream);

/* ------------------------------------------------------------------------------------------
 * Zeroes the listed rows of d_values (float [n_vocab, dim]): for every position i < capacity with 0 <= d_keys[i] <
 * n_vocab, the dim floats of row d_keys[i] become +0.0f.  One launch; a wave per position.  d_keys is a list as
 * gp_row_list_compact writes it: ascending with the sentinel in the tail, so a wave stops at the first key >= n_vocab it
 * meets.  Sentinels write nothing; every row that is not listed keeps its bits.  float4 stores when dim % 4 == 0 and
 * d_values is 16-byte aligned, scalar stores otherwise.
 * GP_ERR_INVALID_ARG: capacity < 1, n_vocab < 1, dim < 1 or n_vocab * dim beyond 63 bits.  GP_ERR_NULL: a pointer missing.
 * ------------------------------------------------------------------------------------------ */
int gp_row_list_zero(int device, const int64_t* d_keys, int64_t capacity, int64_t n_vocab, int32_t dim, float* d_values,
                     void* stream);

#ifdef __cplusplus
}
#endif
