// evaluate.hip -- the head of GRAND+'s evaluation, fused.  Reference: valid() (model.py:158-166) and the
// end of predict() (model.py:218-222), with accuracy() of utils/data_loader.py:161-165:
//
//     logp = log_softmax(z);  loss = nll_loss(logp, y)  (mean over the labels that are not ignore_index)
//     preds = z.argmax(1);    acc = (preds == y).sum() / len(y)
//
// Two kernels, no atomics, no host synchronisation:
//   eval_head_kernel    one wave per evaluated row i: the logits row (row_idx[i], or i) and its label
//                       (labels[label_idx[i]], or labels[i]) give nll, pred and a flag at out_offset + i of three buffers
//                       that successive calls (the batches of valid()) fill;
//   eval_reduce_kernel  stage 1: up to kSlots workgroups, each sums one fixed contiguous slice of nll in float64 and
//                       counts the flags into its own workspace slot (slots nobody owns are zeroed); stage 2: one
//                       workgroup sums the slots in index order with one fixed tree and writes loss, acc and the counts.
// The slices depend on the number of rows only, so the result is bitwise the same run to run and however the rows were
// split into head calls.
#include "eval_head.hpp"                                     // the row arithmetic, shared with eval_tail.hip
#include "eval_plan.hpp"                                     // the slices of the reduction, shared with it too

namespace {

constexpr int kSlots = GP_EVAL_WORKSPACE_BYTES / 40;         // per slot: the f64 sum of nll and four int64 counts

static_assert(kSlots == kBlock * 4, "stage 2 reads four slots per thread");
static_assert(kSlots == gp_eval::kSlots, "eval_plan.hpp cuts the rows for this many slots");

__global__ void __launch_bounds__(kBlock)
eval_head_kernel(HeadArgs a, float* __restrict__ nll, int* __restrict__ pred, unsigned char* __restrict__ flag)
{
    GP_EVAL_HEAD_ROWS(a, nll, pred, flag)
}

// Workspace: sums[kSlots] (f64), then counts[4][kSlots] (int64) = valid, correct, ignored, bad.
// stage 1 (grid = the slices of n): workgroup b sums rows [b * slice, min(n, (b + 1) * slice)) into slot b.
// stage 2 (grid = 1): out = {sum / n_valid, n_correct / n}; 0 / 0 = NaN, as torch's mean of nothing.
__global__ void __launch_bounds__(kBlock)
eval_reduce_kernel(int stage, const float* __restrict__ nll, const unsigned char* __restrict__ flag, long long n, long long slice,
                   double* __restrict__ sums, long long* __restrict__ counts, float* __restrict__ out, long long* __restrict__ out_counts)
{
    __shared__ double lds_d[kWaves];
    __shared__ long long lds_c[kWaves];
    const int tid = threadIdx.x;
    double s = 0.0;
    long long cnt[4] = {0, 0, 0, 0};
    if (stage == 1) {
        const long long first = (long long)blockIdx.x * slice;
        const long long last = first + slice < n ? first + slice : n;
        for (long long i = first + tid; i < last; i += kBlock) {
            s += (double)nll[i];
            const int f = flag[i];
            cnt[0] += f == kWrong || f == kCorrect; cnt[1] += f == kCorrect; cnt[2] += f == kIgnored; cnt[3] += f == kBad;
        }
    } else {
        const double* q = sums + tid * 4;
        s = ((q[0] + q[1]) + q[2]) + q[3];
        for (int k = 0; k < 4; ++k) {
            const long long* c = counts + k * kSlots + tid * 4;
            cnt[k] = c[0] + c[1] + c[2] + c[3];
        }
    }
    s = block_sum<kWaves>(s, lds_d);                         // gp_common.hpp's fixed tree, for the sum and the counts
    for (int k = 0; k < 4; ++k) cnt[k] = block_sum<kWaves>(cnt[k], lds_c);
    if (stage == 1) {
        if (tid == 0) {
            sums[blockIdx.x] = s;
            for (int k = 0; k < 4; ++k) counts[k * kSlots + blockIdx.x] = cnt[k];
        }
        for (int i = gridDim.x + blockIdx.x * kBlock + tid; i < kSlots; i += gridDim.x * kBlock) {
            sums[i] = 0.0;
            for (int k = 0; k < 4; ++k) counts[k * kSlots + i] = 0;
        }
    } else if (tid == 0) {
        out[0] = (float)(s / (double)cnt[0]);
        out[1] = (float)((double)cnt[1] / (double)n);         // len(labels), utils/data_loader.py:165: every row counts
        for (int k = 0; k < 4; ++k) out_counts[k] = cnt[k];
    }
}

}  // namespace

extern "C" {

int gp_eval_head(int device, const float* d_logits, int64_t n_logit_rows, int32_t n_classes, const int64_t* d_row_idx,
                 const int64_t* d_labels, int64_t n_labels, const int64_t* d_label_idx, int64_t n_rows, int64_t ignore_index,
                 int64_t out_offset, int64_t out_capacity, float* d_nll, int32_t* d_pred, uint8_t* d_flag, void* stream)
{
    const char* where = "gp_eval_head";
    if (n_classes < 1 || n_classes > kMaxC || n_rows < 0 || n_logit_rows < 0 || n_labels < 0 || out_offset < 0 ||
        out_capacity < 0 || n_rows > out_capacity || out_offset > out_capacity - n_rows)
        return fail(GP_ERR_INVALID_ARG, where,
                    "n_classes outside [1, 4096], a negative size or offset, or out_offset + n_rows past out_capacity");
    if ((!d_row_idx && n_rows > n_logit_rows) || (!d_label_idx && n_rows > n_labels))
        return fail(GP_ERR_INVALID_ARG, where, "without an index list n_rows may not exceed n_logit_rows / n_labels");
    if (n_rows == 0) return GP_OK;
    if ((n_logit_rows > 0 && !d_logits) || (n_labels > 0 && !d_labels) || !d_nll || !d_pred || !d_flag)
        return fail(GP_ERR_NULL, where, "a device pointer is NULL");
    if (const int rc = set_device(device, where)) return rc;
    const HeadArgs a = {d_logits, (long long)n_logit_rows, n_classes, (const long long*)d_row_idx, (const long long*)d_labels,
                        (long long)n_labels, (const long long*)d_label_idx, (long long)n_rows, (long long)ignore_index,
                        (long long)out_offset};
    hipLaunchKernelGGL(eval_head_kernel, dim3(row_grid(n_rows, kWaves)), dim3(kBlock), 0, (hipStream_t)stream, a, d_nll, (int*)d_pred,
                       (unsigned char*)d_flag);
    return launch_status("eval_head_kernel");
}

int gp_eval_reduce(int device, const float* d_nll, const uint8_t* d_flag, int64_t n_rows, void* d_workspace, float* d_out,
                   int64_t* d_counts, void* stream)
{
    const char* where = "gp_eval_reduce";
    if (n_rows < 0) return fail(GP_ERR_INVALID_ARG, where, "n_rows < 0");
    if ((n_rows > 0 && (!d_nll || !d_flag)) || !d_workspace || !d_out || !d_counts)
        return fail(GP_ERR_NULL, where, "a device pointer is NULL");
    if (const int rc = set_device(device, where)) return rc;
    hipStream_t s = (hipStream_t)stream;
    double* sums = static_cast<double*>(d_workspace);
    long long* counts = reinterpret_cast<long long*>(sums + kSlots);
    const gp_eval::ReducePlan plan = gp_eval::reduce_plan(n_rows);          // the slices follow from n_rows alone
    const long long grid = plan.grid, slice = plan.slice;
    hipLaunchKernelGGL(eval_reduce_kernel, dim3((int)grid), dim3(kBlock), 0, s, 1, d_nll, (const unsigned char*)d_flag,
                       (long long)n_rows, slice, sums, counts, (float*)nullptr, (long long*)nullptr);
    if (const int rc = launch_status("eval_reduce_kernel (stage 1)")) return rc;
    hipLaunchKernelGGL(eval_reduce_kernel, dim3(1), dim3(kBlock), 0, s, 2, (const float*)nullptr, (const unsigned char*)nullptr,
                       (long long)n_rows, slice, sums, counts, d_out, (long long*)d_counts);
    return launch_status("eval_reduce_kernel (stage 2)");
}

}  // extern "C"
