/*
 * grandplus_eval.h -- the evaluation entry points of the C ABI (implemented by grand_plus_amd/csrc/evaluate.hip).
 *
 * Part of the ABI that grandplus.h describes (GP_ABI_VERSION and the status codes are defined there): grandplus.h
 * includes this file, so callers include grandplus.h alone.  The ctypes binding declares these entry points under this
 * file's name in _native.ABI, and tests/test_host_abi.py holds that table against this file type by type.
 */
#ifndef GRANDPLUS_EVAL_H
#define GRANDPLUS_EVAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * The head of an evaluation, fused (valid() model.py:158-166, predict() model.py:218-222, accuracy()
 * utils/data_loader.py:161-165):
 *
 *     logp = log_softmax(z);  loss = nll_loss(logp, y);  preds = z.argmax(1);  acc = (preds == y).sum() / len(y)
 *
 * gp_eval_head, for i < n_rows: the logits row r = d_row_idx[i] (NULL: r = i) of d_logits fp32 [n_logit_rows x n_classes]
 * (1 <= n_classes <= 4096) and the label y = d_labels[d_label_idx[i]] (NULL: d_labels[i]; d_labels int64 [n_labels]) give,
 * at index out_offset + i of three buffers of out_capacity entries that successive calls fill:
 *   d_nll  fp32   -logp[y], logp = (z - max) - log(sum exp(z - max)) in fp32; 0 for a row that is ignored or bad;
 *   d_pred int32  the first index of the row's largest logit, a NaN counting as the largest (torch.argmax, numpy.argmax);
 *                 -1 when r is outside [0, n_logit_rows);
 *   d_flag uint8  GP_EVAL_WRONG, GP_EVAL_CORRECT (pred == y), GP_EVAL_IGNORED (y == ignore_index) or GP_EVAL_BAD: another
 *                 label outside [0, n_classes), or an index outside its array.  A bad value is never used as an address;
 *                 it is counted, and nothing asserts on the device.
 * One launch, one wave per row.  Without an index list n_rows may not exceed the array's length.
 *
 * gp_eval_reduce over the first n_rows entries of d_nll and d_flag writes d_out fp32[2] = {loss = sum(nll) / n_valid,
 * acc = n_correct / n_rows} (every row counts in the accuracy's denominator, ignored and bad ones too: len(labels) of
 * utils/data_loader.py:165) and d_counts int64[4] = {n_valid, n_correct, n_ignored, n_bad}.  n_valid = 0 gives a NaN loss
 * (torch's mean of nothing), n_rows = 0 a NaN accuracy.  d_workspace: GP_EVAL_WORKSPACE_BYTES bytes of device memory,
 * 8-byte aligned, the caller's.  Two launches: up to 1024 workgroups each sum one contiguous slice of d_nll in float64
 * into its own slot, then one workgroup sums the slots in index order.
 *
 * Contracts:
 *   - no atomics; the slices follow from n_rows alone, so d_out is bitwise the same run to run and however the rows
 *     were split into gp_eval_head calls;
 *   - nothing on the call path synchronises, copies or allocates; both enqueue on `stream`;
 *   - arguments are checked before the device is touched: GP_ERR_INVALID_ARG for n_classes outside [1, 4096], a negative
 *     size or offset, out_offset + n_rows > out_capacity, or n_rows past an array that has no index list; GP_ERR_NULL
 *     for a missing pointer.
 * ------------------------------------------------------------------------------------------ */
#define GP_EVAL_WRONG 0
#define GP_EVAL_CORRECT 1
#define GP_EVAL_IGNORED 2
#define GP_EVAL_BAD 3
#define GP_EVAL_WORKSPACE_BYTES (1024 * 40)   /* 1024 slots of one float64 sum and four int64 counts */

int gp_eval_head(int device, const float* d_logits, int64_t n_logit_rows, int32_t n_classes, const int64_t* d_row_idx,
                 const int64_t* d_labels, int64_t n_labels, const int64_t* d_label_idx, int64_t n_rows, int64_t ignore_index,
                 int64_t out_offset, int64_t out_capacity, float* d_nll, int32_t* d_pred, uint8_t* d_flag, void* stream);
int gp_eval_reduce(int device, const float* d_nll, const uint8_t* d_flag, int64_t n_rows, void* d_workspace, float* d_out,
                   int64_t* d_counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GRANDPLUS_EVAL_H */
