// eval_tail.hip -- the evaluation's head and its reduction as one launch: what gp_eval_head at offset 0
// followed by gp_eval_reduce (evaluate.hip) writes in three launches, bit for bit.
//
//   head    every workgroup: one wave per row, eval_head.hpp's rows on eval_head_kernel's grid;
//   ticket  every workgroup: all waves drain their stores, a barrier, then thread 0 releases at agent scope and draws a
//           ticket with one relaxed agent-scope fetch_add; the workgroup that draws gridDim.x - 1 has seen every other
//           workgroup's release, acquires at agent scope and goes on.  Nobody waits: a workgroup that is not last returns;
//   reduce  the last workgroup alone: for each slice of eval_plan.hpp in index order, eval_reduce_kernel's stage 1 (thread
//           tid sums rows first + tid, + 256, ... in float64, block_sum) into an LDS slot; then its stage 2 over the slots
//           (four per thread, ((q0 + q1) + q2) + q3, block_sum).  Slots past the slices hold zeros, as the workspace of
//           gp_eval_reduce does, and threads whose four slots are past kTailSlices add the same zeros.
// The ticket decides which workgroup reduces, never what is added in what order.
#include "eval_head.hpp"
#include "eval_plan.hpp"
#include "eval_tail_abi.hpp"

namespace {

constexpr int kTailSlices = gp_eval::kTailSlices;

static_assert(GP_EVAL_TAIL_MAX_ROWS == gp_eval::kTailMaxRows && GP_EVAL_TAIL_WORKSPACE_BYTES == gp_eval::kTailWorkspaceBytes,
              "eval_tail_abi.hpp and eval_plan.hpp state the same cap and workspace");
static_assert(kTailSlices % 4 == 0 && kTailSlices <= gp_eval::kSlots && kTailSlices <= kBlock * 4, "stage 2 reads four slots per thread");

struct TailLds {                                             // one LDS object: the trees' scratch, the slots, the flag
    double d[kWaves];
    long long c[kWaves];
    double sums[kTailSlices];
    long long counts[4][kTailSlices];
    int last;
};

__global__ void __launch_bounds__(kBlock)
eval_tail_kernel(HeadArgs a, float* nll, int* pred, unsigned char* flag, unsigned int* ticket, int n_slices, long long slice,
                 float* __restrict__ out, long long* __restrict__ out_counts)
{
    __shared__ TailLds lds;
    const int tid = threadIdx.x;
    GP_EVAL_HEAD_ROWS(a, nll, pred, flag)

    // publish this workgroup's rows, then draw the ticket: one release per workgroup, fence before the fetch_add
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned int t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = t == gridDim.x - 1;
        if (last) {                                          // one acquire, in the reducer alone
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        lds.last = last;
    }
    __syncthreads();
    if (!lds.last) return;                                   // workgroup-uniform

    // stage 1 of eval_reduce_kernel, slice after slice
    for (int b = 0; b < n_slices; ++b) {
        const long long first = (long long)b * slice;
        const long long end = first + slice < a.n ? first + slice : a.n;
        double s = 0.0;
        long long cnt[4] = {0, 0, 0, 0};
        for (long long i = first + tid; i < end; i += kBlock) {
            s += (double)nll[i];
            const int f = flag[i];
            cnt[0] += f == kWrong || f == kCorrect; cnt[1] += f == kCorrect; cnt[2] += f == kIgnored; cnt[3] += f == kBad;
        }
        s = block_sum<kWaves>(s, lds.d);
        for (int k = 0; k < 4; ++k) cnt[k] = block_sum<kWaves>(cnt[k], lds.c);
        if (tid == 0) {
            lds.sums[b] = s;
            for (int k = 0; k < 4; ++k) lds.counts[k][b] = cnt[k];
        }
    }
    for (int i = n_slices + tid; i < kTailSlices; i += kBlock) {
        lds.sums[i] = 0.0;
        for (int k = 0; k < 4; ++k) lds.counts[k][i] = 0;
    }
    __syncthreads();

    // stage 2: four slots per thread in index order, one fixed tree
    double s = 0.0;
    long long cnt[4] = {0, 0, 0, 0};
    if (tid * 4 < kTailSlices) {
        const double* q = lds.sums + tid * 4;
        s = ((q[0] + q[1]) + q[2]) + q[3];
        for (int k = 0; k < 4; ++k) {
            const long long* c = lds.counts[k] + tid * 4;
            cnt[k] = c[0] + c[1] + c[2] + c[3];
        }
    }
    s = block_sum<kWaves>(s, lds.d);
    for (int k = 0; k < 4; ++k) cnt[k] = block_sum<kWaves>(cnt[k], lds.c);
    if (tid == 0) {
        out[0] = (float)(s / (double)cnt[0]);
        out[1] = (float)((double)cnt[1] / (double)a.n);      // len(labels), utils/data_loader.py:165: every row counts
        for (int k = 0; k < 4; ++k) out_counts[k] = cnt[k];
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next call starts from zero
    }
}

}  // namespace

extern "C" {

int gp_eval_tail(int device, const float* d_logits, int64_t n_logit_rows, int32_t n_classes, const int64_t* d_row_idx,
                 const int64_t* d_labels, int64_t n_labels, const int64_t* d_label_idx, int64_t n_rows, int64_t ignore_index,
                 float* d_nll, int32_t* d_pred, uint8_t* d_flag, void* d_workspace, float* d_out, int64_t* d_counts, void* stream)
{
    const char* where = "gp_eval_tail";
    if (n_classes < 1 || n_classes > kMaxC || n_rows < 0 || n_logit_rows < 0 || n_labels < 0)
        return fail(GP_ERR_INVALID_ARG, where, "n_classes outside [1, 4096] or a negative size");
    if (n_rows > GP_EVAL_TAIL_MAX_ROWS)
        return fail(GP_ERR_INVALID_ARG, where, "n_rows above GP_EVAL_TAIL_MAX_ROWS: run gp_eval_head and gp_eval_reduce");
    if ((!d_row_idx && n_rows > n_logit_rows) || (!d_label_idx && n_rows > n_labels))
        return fail(GP_ERR_INVALID_ARG, where, "without an index list n_rows may not exceed n_logit_rows / n_labels");
    if ((uintptr_t)d_workspace % 4)
        return fail(GP_ERR_INVALID_ARG, where, "d_workspace is not 4-byte aligned");
    if (!d_workspace || !d_out || !d_counts ||
        (n_rows > 0 && ((n_logit_rows > 0 && !d_logits) || (n_labels > 0 && !d_labels) || !d_nll || !d_pred || !d_flag)))
        return fail(GP_ERR_NULL, where, "a device pointer is NULL");
    if (const int rc = set_device(device, where)) return rc;
    const HeadArgs a = {d_logits, (long long)n_logit_rows, n_classes, (const long long*)d_row_idx, (const long long*)d_labels,
                        (long long)n_labels, (const long long*)d_label_idx, (long long)n_rows, (long long)ignore_index, 0};
    const gp_eval::ReducePlan plan = gp_eval::reduce_plan(n_rows);          // at most kTailSlices slices under the cap
    hipLaunchKernelGGL(eval_tail_kernel, dim3(row_grid(n_rows, kWaves)), dim3(kBlock), 0, (hipStream_t)stream, a, d_nll, (int*)d_pred,
                       (unsigned char*)d_flag, (unsigned int*)d_workspace, (int)plan.grid, plan.slice, d_out, (long long*)d_counts);
    return launch_status("eval_tail_kernel");
}

}  // extern "C"
