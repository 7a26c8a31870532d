/*
 * optim_rows_abi.hpp -- the entry points of the embedding table's row-list optimiser step (implemented by
 * csrc/optim_rows.hip).
 *
 * NOT part of C ABI 4: these are extern "C" symbols of libgrandplus.so that no public header declares, as
 * mag_det_abi.hpp's.  The one caller is grand_plus_amd/optim_rows.py; _native.PRIVATE_ABI binds them, under this file's
 * name and the convention of _native.ABI: d_* and void* travel as c_void_p, scalars map one to one.
 * tests/test_host_abi.py holds that table against this file.
 *
 * The table is d_param float [n_vocab, dim] with Adam's d_exp_avg and d_exp_avg_sq of the same shape.  Its gradient is
 * d_dW float [n_vocab, dim] TOGETHER WITH d_keys int64 [n_sorted], ascending: the sorted key list of
 * gp_mag_prop_rows_backward_det (mag_det_abi.hpp).  Row r of d_dW holds a gradient only when r is TOUCHED, that is when
 * some position i has d_keys[i] == r (csrc/optim_rows_layout.hpp states the rule); every other row of d_dW holds
 * anything at all -- it was never zeroed -- and is never read.  The gradient of an untouched row is 0.
 *
 * d_workspace is gp_clip_adam_step's (GP_OPTIM_WORKSPACE_BYTES: 1 024 float64 partials of the squared norm), so that one
 * norm is taken over the dense tensors (gp_clip_adam_step with GP_OPTIM_NORM_ONLY) and the table together.
 *
 * Common contract: arguments are checked before the device is touched; nothing on a call path reads a device value on the
 * host, allocates, copies or synchronises, so every launch can be captured; no atomics; all offsets are 64-bit.
 */
#pragma once

#include <stdint.h>

#include "grandplus.h"

#define GP_OPTIM_ROWS_EXACT 1   /* every element of the table gets the dense update, untouched rows with g = 0.0f */
#define GP_OPTIM_ROWS_LAZY 2    /* touched rows alone; every other row of the table and of Adam's state keeps its bits */

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * The table's share of the squared gradient norm: one launch on `stream`.  A wave takes a window of 64 positions of
 * d_keys; a workgroup sums the squares (in float64, where an fp32 square is exact) of the dim elements of every touched
 * row whose head lies in its windows, in a fixed order, and leaves the sum in workspace slot blockIdx.x.
 * accumulate = 0: the first launch into the workspace; it writes its slots and zeroes every other.  accumulate != 0: the
 * sum is added to what the slot holds (after gp_clip_adam_step(GP_OPTIM_NORM_ONLY) over the dense gradients).
 * n_sorted = 0 is valid: with accumulate = 0 the workspace is zeroed, otherwise nothing is launched.
 * GP_ERR_INVALID_ARG: n_sorted < 0, n_vocab < 1, dim < 1.  GP_ERR_NULL: d_keys, d_dW or d_workspace missing.
 * ------------------------------------------------------------------------------------------ */
int gp_optim_rows_sqnorm(int device, const int64_t* d_keys, int64_t n_sorted, int64_t n_vocab, int32_t dim,
                         const float* d_dW, int accumulate, void* d_workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * The clip coefficient and the Adam update of the table: gp_clip_adam_step(GP_OPTIM_NORM_READY) for one tensor whose
 * gradient is (d_dW, d_keys).  One launch.  The workspace holds the squared norm's partials (the call above, and
 * gp_clip_adam_step(GP_OPTIM_NORM_ONLY) before it if there are dense gradients); *d_norm_out = the norm before clipping.
 * The hyper-parameters, step_size and rsqrt_bc2 are gp_clip_adam_step's; so is the arithmetic of an element
 * (csrc/optim_math.hpp), with nothing fused (-ffp-contract=off).
 *   mode = GP_OPTIM_ROWS_EXACT: every element of the table is updated, with g = d_dW[r, h] for a touched row and the
 *     literal 0.0f for every other: bit for bit gp_clip_adam_step on a zero-filled dense gradient that holds the touched
 *     rows, a non-finite coefficient included (0.0f * NaN is NaN there and here).  d_dW of an untouched row is not loaded.
 *   mode = GP_OPTIM_ROWS_LAZY: only the touched rows of d_param, d_exp_avg and d_exp_avg_sq are read and written, each
 *     element by the same update; every other row keeps its bits.  This is NOT the reference's trajectory: under
 *     torch.optim.Adam (model_mag.py:312) an untouched row still moves while its moments decay.  weight_decay must be 0:
 *     a decay applied to touched rows alone is nobody's semantics (GP_ERR_INVALID_ARG).
 * n_sorted = 0 is valid: exact mode runs the zero-gradient update of the whole table; lazy mode launches nothing (and
 * leaves *d_norm_out alone).
 * GP_ERR_INVALID_ARG: an unknown mode, n_sorted < 0, n_vocab < 1, dim < 1, a hyper-parameter that is not finite, lazy mode
 * with weight_decay != 0.  GP_ERR_NULL: a pointer missing.
 * ------------------------------------------------------------------------------------------ */
int gp_clip_adam_rows(int device, float* d_param, float* d_exp_avg, float* d_exp_avg_sq, const float* d_dW,
                      const int64_t* d_keys, int64_t n_sorted, int64_t n_vocab, int32_t dim, int mode, float max_norm,
                      float lr, double beta1, double beta2, float eps, float weight_decay, float step_size, float rsqrt_bc2,
                      void* d_workspace, float* d_norm_out, void* stream);

/* The same with step_size and rsqrt_bc2 read on the device, as gp_clip_adam_step_dev reads them (two floats of a
 * gp_step_state): GP_ERR_NULL when either is missing. */
int gp_clip_adam_rows_dev(int device, float* d_param, float* d_exp_avg, float* d_exp_avg_sq, const float* d_dW,
                          const int64_t* d_keys, int64_t n_sorted, int64_t n_vocab, int32_t dim, int mode, float max_norm,
                          float lr, double beta1, double beta2, float eps, float weight_decay, const float* d_step_size,
                          const float* d_rsqrt_bc2, void* d_workspace, float* d_norm_out, void* stream);

#ifdef __cplusplus
}
#endif
