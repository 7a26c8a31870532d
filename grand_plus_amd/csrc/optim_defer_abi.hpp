/*
 * optim_defer_abi.hpp -- the entry points of the embedding table's deferred exact Adam step (implemented by
 * csrc/optim_defer.hip).
 *
 * NOT part of C ABI 4: these are extern "C" symbols of libgrandplus.so that no public header declares, as
 * optim_rows_abi.hpp's.  The one caller is grand_plus_amd/optim_rows.py; _native.PRIVATE_ABI binds them, under this file's
 * name and the convention of _native.ABI: d_* and void* travel as c_void_p, scalars map one to one.
 * tests/test_host_abi.py holds that table against this file.
 *
 * The table, Adam's two moments, the gradient (d_dW with d_keys) and the workspace are optim_rows_abi.hpp's.  d_keys is
 * either kind of list that exists: the deterministic backward's sorted key list (duplicates; a row's HEAD is the first
 * position of its run, csrc/optim_rows_layout.hpp) or the bitmap list (each row once); ascending, sentinel n_vocab in the
 * tail.  The deferred state (csrc/optim_defer_layout.hpp states every rule):
 *   d_last  int32 [n_vocab]: row r is current through step d_last[r];
 *   d_hist  a ring of `capacity` 16-byte entries {float step_size, float rsqrt_bc2, float coef, uint32 tag}, the entry of
 *           step s in slot s % capacity; capacity is a power of two in [4, 65536];
 *   d_flag  int32 [1]: bit 1 (value 2) is set, with a plain store, when a row could not be served; never cleared here;
 *   d_tick  the address of a gp_step_state's tick (uint64): T, the step that is running (after gp_step_advance) or that
 *           ran last.  It is read on the device.
 * A row is SERVED at tick T when 0 <= d_last[r] <= T, T < 2^31, T - d_last[r] <= capacity and every ring slot its replay
 * reads carries the tag of the step it should hold.  A served row that lags gets the zero-gradient update of every step
 * it missed, in order, through csrc/optim_math.hpp's adam_element with the literal 0.0f and that step's entry: the bits the
 * dense step gives it (-ffp-contract=off).  An unserved row keeps its bits in d_param, both moments and d_last.
 *
 * Common contract: arguments are checked before the device is touched; nothing on a call path reads a device value on the
 * host, allocates, copies or synchronises, so every launch can be captured; no atomics; all offsets are 64-bit.
 * GP_ERR_INVALID_ARG for every entry: n_vocab < 1, dim < 1, n_vocab * dim beyond 63 bits, a capacity that is no power of
 * two in [4, 65536], a hyper-parameter that is not finite; where there is a list, n_sorted < 0.  GP_ERR_NULL: a pointer
 * missing.
 */
#pragma once

#include <stdint.h>

#include "grandplus.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Before the forward of step T: every row that has a head in d_keys is brought through step T - 1, and d_last[r] = T - 1.
 * One launch on `stream`; a wave per list position, heads alone do work.  Rows that are not listed keep every bit.
 * n_sorted = 0 is GP_OK with nothing launched.
 * ------------------------------------------------------------------------------------------ */
int gp_optim_defer_catch_up(int device, float* d_param, float* d_exp_avg, float* d_exp_avg_sq, const int64_t* d_keys,
                            int64_t n_sorted, int64_t n_vocab, int32_t dim, double beta1, double beta2, float eps,
                            float weight_decay, const uint64_t* d_tick, int32_t* d_last, const void* d_hist, int32_t capacity,
                            int32_t* d_flag, void* stream);

/* ------------------------------------------------------------------------------------------
 * The table's clip + Adam step of step T over the touched rows: gp_clip_adam_rows_dev's arguments and norm contract
 * (the workspace holds the squared norm's partials; *d_norm_out = the norm before clipping), without a mode.  One launch.
 * Workgroup 0 writes the ring entry of step T -- step_size and rsqrt_bc2 as read from the two device addresses, coef as
 * the workspace gives it, tag T -- so the launch happens with n_sorted = 0 too: an empty batch is still a step of history.
 * Every head row is first brought through T - 1 (normally no trip: gp_optim_defer_catch_up ran before the forward), then
 * takes adam_element with its row of d_dW, then d_last[r] = T.  An unserved row is not stepped.
 * weight_decay needs no special case: the replay applies it at every step, as the dense step does.
 * ------------------------------------------------------------------------------------------ */
int gp_optim_defer_step(int device, float* d_param, float* d_exp_avg, float* d_exp_avg_sq, const float* d_dW,
                        const int64_t* d_keys, int64_t n_sorted, int64_t n_vocab, int32_t dim, float max_norm, float lr,
                        double beta1, double beta2, float eps, float weight_decay, const float* d_step_size,
                        const float* d_rsqrt_bc2, const uint64_t* d_tick, int32_t* d_last, void* d_hist, int32_t capacity,
                        int32_t* d_flag, void* d_workspace, float* d_norm_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Every row of the table is brought through step T, and d_last[r] = T: afterwards d_param and both moments hold what the
 * dense step holds after step T.  One launch over a capped grid; a wave takes 64 rows at a time, and a row that is
 * current costs the 4-byte read of its d_last.  A second flush at the same tick changes no bit.
 * ------------------------------------------------------------------------------------------ */
int gp_optim_defer_flush(int device, float* d_param, float* d_exp_avg, float* d_exp_avg_sq, int64_t n_vocab, int32_t dim,
                         double beta1, double beta2, float eps, float weight_decay, const uint64_t* d_tick, int32_t* d_last,
                         const void* d_hist, int32_t capacity, int32_t* d_flag, void* stream);

#ifdef __cplusplus
}
#endif
