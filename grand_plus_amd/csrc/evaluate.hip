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
#include "gp_common.hpp"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxC = 4096;
constexpr int kSlots = GP_EVAL_WORKSPACE_BYTES / 40;         // per slot: the f64 sum of nll and four int64 counts
constexpr int kMinSlice = 1024;                              // rows of a stage-1 workgroup, at least

static_assert(kSlots == kBlock * 4, "stage 2 reads four slots per thread");

enum { kWrong = GP_EVAL_WRONG, kCorrect = GP_EVAL_CORRECT, kIgnored = GP_EVAL_IGNORED, kBad = GP_EVAL_BAD };   // a row's flag

struct HeadArgs {
    const float* z;                 // [n_z x C]
    long long n_z; int C;
    const long long* row_idx;       // [n] or NULL
    const long long* labels;        // [n_labels]
    long long n_labels;
    const long long* label_idx;     // [n] or NULL
    long long n, ignore, offset;
};

// torch.argmax / numpy.argmax: the first index of the largest value, where a NaN is larger than every number
__device__ __forceinline__ bool better(float a, int ia, float b, int ib)
{
    if (a != a) return b != b ? ia < ib : true;
    if (b != b) return false;
    return a > b || (a == b && ia < ib);
}

__global__ void __launch_bounds__(kBlock)
eval_head_kernel(HeadArgs a, float* __restrict__ nll, int* __restrict__ pred, unsigned char* __restrict__ flag)
{
    const int lane = threadIdx.x & 63;
    const long long n_waves = (long long)gridDim.x * kWaves;
    for (long long i = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6); i < a.n; i += n_waves) {   // wave-uniform
        const long long r = a.row_idx ? a.row_idx[i] : i;
        const long long l = a.label_idx ? a.label_idx[i] : i;
        float loss = 0.0f; int arg = -1; int fl = kBad;
        if (r >= 0 && r < a.n_z) {                            // an index outside its array is never used as an address
            const float* __restrict__ zr = a.z + (size_t)r * a.C;
            // the first 64 classes stay in a register: one read of the row for C <= 64
            const float z0 = lane < a.C ? zr[lane] : -INFINITY;
            float best = z0; arg = lane < a.C ? lane : 0x7FFFFFFF;
            for (int c = lane + 64; c < a.C; c += 64) {
                const float v = zr[c];
                if (better(v, c, best, arg)) { best = v; arg = c; }
            }
            for (int o = 32; o > 0; o >>= 1) {
                const float ob = __shfl_xor(best, o); const int oa = __shfl_xor(arg, o);
                if (better(ob, oa, best, arg)) { best = ob; arg = oa; }
            }
            if (l >= 0 && l < a.n_labels) {
                const long long y = a.labels[l];
                if (y == a.ignore) fl = kIgnored;
                else if (y >= 0 && y < a.C) {
                    // (z - max) - log sum exp(z - max), the objective's order; a NaN in the row is the max: NaN, as torch
                    float e = lane < a.C ? expf(z0 - best) : 0.0f;
                    for (int c = lane + 64; c < a.C; c += 64) e += expf(zr[c] - best);
                    const float ls = logf(wave_sum(e));
                    loss = -((zr[y] - best) - ls);
                    fl = arg == y ? kCorrect : kWrong;
                }
            }
        }
        if (lane == 0) { nll[a.offset + i] = loss; pred[a.offset + i] = arg; flag[a.offset + i] = (unsigned char)fl; }
    }
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
    // the slices follow from n_rows alone: at least kMinSlice rows each, at most kSlots of them
    long long grid = (n_rows + kMinSlice - 1) / kMinSlice;
    grid = grid < 1 ? 1 : grid > kSlots ? kSlots : grid;
    const long long slice = (n_rows + grid - 1) / grid;
    hipLaunchKernelGGL(eval_reduce_kernel, dim3((int)grid), dim3(kBlock), 0, s, 1, d_nll, (const unsigned char*)d_flag,
                       (long long)n_rows, slice, sums, counts, (float*)nullptr, (long long*)nullptr);
    if (const int rc = launch_status("eval_reduce_kernel (stage 1)")) return rc;
    hipLaunchKernelGGL(eval_reduce_kernel, dim3(1), dim3(kBlock), 0, s, 2, (const float*)nullptr, (const unsigned char*)nullptr,
                       (long long)n_rows, slice, sums, counts, d_out, (long long*)d_counts);
    return launch_status("eval_reduce_kernel (stage 2)");
}

}  // extern "C"
