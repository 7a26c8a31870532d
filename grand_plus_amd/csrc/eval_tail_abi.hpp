/*
 * eval_tail_abi.hpp -- the evaluation's head and reduction as one launch (implemented by csrc/eval_tail.hip).
 *
 * NOT part of C ABI 4: an extern "C" symbol of libgrandplus.so that no public header declares, as fit_rows_abi.hpp's and
 * row_mark_abi.hpp's.  The one caller is grand_plus_amd/evaluate.py; _native.PRIVATE_ABI binds it, under this file's name
 * and the convention of _native.ABI: d_* and void* travel as c_void_p, scalars map one to one.  tests/test_host_abi.py
 * holds that table against this file.  grandplus_eval.h stays as it is.
 */
#pragma once

#include <stdint.h>

#include "grandplus.h"

/* the most rows of one call: 64 slices of 1024 rows (csrc/eval_plan.hpp), which the last workgroup walks one after another */
#define GP_EVAL_TAIL_MAX_ROWS 65536
/* d_workspace: the ticket counter (one uint32 at offset 0), padded.  The slot sums live in LDS, not here.  The caller
 * zeroes it ONCE, when it allocates it; every call leaves it zero. */
#define GP_EVAL_TAIL_WORKSPACE_BYTES 64

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * gp_eval_head at out_offset 0 over n_rows (out_capacity = n_rows), then gp_eval_reduce over those rows, as ONE launch on
 * `stream`.  d_nll, d_pred, d_flag [n_rows], d_out [2] and d_counts [4] are bit for bit what those two calls write:
 * the same row arithmetic (csrc/eval_head.hpp) on the same grid, the same slices (csrc/eval_plan.hpp), the same float64
 * sums in the same order.  The workgroup that finishes last reduces: every workgroup draws a ticket from the counter in
 * d_workspace once its rows are stored and released, and the one that draws the last ticket acquires and sums.  The ticket
 * decides who reduces, never what is added in what order, so the result is bitwise the same from run to run.  Nothing waits
 * or spins.  The reducer stores 0 to the counter before it exits.
 * n_rows = 0 writes the NaN loss and NaN accuracy of gp_eval_reduce and zero counts.
 * Arguments are checked before the device is touched, with gp_eval_head's codes.  GP_ERR_INVALID_ARG: n_classes outside
 * [1, 4096], a negative size, n_rows > GP_EVAL_TAIL_MAX_ROWS (run gp_eval_head and gp_eval_reduce there), n_rows above
 * n_logit_rows / n_labels without the index list, or a d_workspace that is not 4-byte aligned.  GP_ERR_NULL: d_workspace,
 * d_out or d_counts missing, or with n_rows > 0 one of d_nll, d_pred, d_flag, d_logits (n_logit_rows > 0), d_labels
 * (n_labels > 0).  Nothing on the call path allocates, copies or synchronises: the launch can be captured.
 * ------------------------------------------------------------------------------------------ */
int gp_eval_tail(int device, const float* d_logits, int64_t n_logit_rows, int32_t n_classes, const int64_t* d_row_idx,
                 const int64_t* d_labels, int64_t n_labels, const int64_t* d_label_idx, int64_t n_rows, int64_t ignore_index,
                 float* d_nll, int32_t* d_pred, uint8_t* d_flag, void* d_workspace, float* d_out, int64_t* d_counts, void* stream);

#ifdef __cplusplus
}
#endif
