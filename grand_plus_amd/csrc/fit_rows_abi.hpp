/*
 * fit_rows_abi.hpp -- the dirty-row snapshot of an embedding table for the fit loop (implemented by
 * csrc/fit_rows.hip).
 *
 * NOT part of C ABI 4: these are extern "C" symbols of libgrandplus.so that no public header declares, as
 * mag_det_abi.hpp's, optim_rows_abi.hpp's and row_mark_abi.hpp's.  The one caller is grand_plus_amd/fit.py;
 * _native.PRIVATE_ABI binds them, under this file's name and the convention of _native.ABI: d_* and void* travel as
 * c_void_p, scalars map one to one.  tests/test_host_abi.py holds that table against this file.
 *
 * gp_fit_snapshot (grandplus_fit.h) copies every tensor of the model whole when the early-stop rule takes a new best.
 * Under the lazy table step (optim_rows_abi.hpp) only the rows a batch's bags name ever change, and the row lists of
 * DESIGN §7t and §7u say which.  Here those rows are collected in a bitmap of n_vocab bits between two snapshots
 * (csrc/row_mark_layout.hpp states the layout; csrc/fit_rows_layout.hpp which wave owns which word), and the snapshot
 * copies the rows whose bit is set, then clears the bits.  The invariant the caller keeps: every row whose bit is 0 has the
 * same bits in the table and in its snapshot.  A set bit too many only copies a row too many.
 *
 * d_dirty is int32 [(n_vocab + 31) / 32].
 *
 * Common contract: arguments are checked before the device is touched -- the sizes first, then the pointers; nothing on a
 * call path reads a device value on the host, allocates, copies or synchronises, so every launch can be captured; all
 * offsets are 64-bit.
 */
#pragma once

#include <stdint.h>

#include "grandplus.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Marks the rows of a key list as dirty.  One launch on `stream`.  For every i < n_keys with 0 <= d_keys[i] < n_vocab, bit
 * d_keys[i] of d_dirty is set with an atomic OR; every other key (a negative one, the sentinel n_vocab of a list's tail,
 * anything above it) marks nothing and is never used as an address.  d_keys is a row list as the table gradient hands it
 * over: the sorted keys of gp_mag_det_keys (duplicates) or the list of gp_row_list_compact (each row once); a key equal to
 * the one before it is skipped, the first of the run marks.  Bits already set stay set.  The result is the same from run
 * to run: an OR is idempotent and commutative.
 * GP_ERR_INVALID_ARG: n_vocab < 1, n_keys < 0 or a pointer that is not 4-byte aligned.  GP_ERR_NULL: a pointer missing.
 * n_keys = 0 is GP_OK with nothing launched.
 * ------------------------------------------------------------------------------------------ */
int gp_fit_rows_mark(int device, const int64_t* d_keys, int64_t n_keys, int64_t n_vocab, int32_t* d_dirty, void* stream);

/* ------------------------------------------------------------------------------------------
 * Copies the dirty rows of d_src (n_vocab rows of dim 32-bit words) to d_dst when d_track->copy_now != 0, and does
 * nothing otherwise: then nothing but that field is read, and d_dirty keeps its bits.  One launch on `stream`, to be issued
 * after gp_fit_track_update as a launch of its own (the reason grandplus_fit.h gives for gp_fit_snapshot: every workgroup
 * reads a decision made before the copy began).  No atomics.
 * Every word of d_dirty is owned by exactly one wave of a capped grid (csrc/fit_rows_layout.hpp); the wave reads its word,
 * copies row r for every set bit r < n_vocab as bits -- a NaN keeps its payload -- and stores 0 to the word.  A bit at or
 * above n_vocab copies nothing and is cleared.  16-byte loads and stores when dim % 4 == 0 and d_src and d_dst are 16-byte
 * aligned, 4-byte ones otherwise.  Every row whose bit was 0 keeps its bits in d_dst.
 * GP_ERR_INVALID_ARG: n_vocab < 1, dim < 1, n_vocab * dim beyond 63 bits or a pointer that is not 4-byte aligned.
 * GP_ERR_NULL: a pointer missing.
 * ------------------------------------------------------------------------------------------ */
int gp_fit_rows_snapshot(int device, const gp_fit_track* d_track, const void* d_src, void* d_dst, int64_t n_vocab, int32_t dim,
                         int32_t* d_dirty, void* stream);

#ifdef __cplusplus
}
#endif
