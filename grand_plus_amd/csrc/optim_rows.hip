// optim_rows.hip -- DESIGN §7t: the clip + Adam step of MAG's embedding table over the rows a batch touched.
//
// The dense step (optim.hip, §7g) reads a [V, H] gradient twice -- once for the norm, once for the update -- after Python
// has zero-filled it, although a batch touches a small part of the table and the deterministic backward (mag_det.hip, §7o)
// knows which: it holds the sorted key list, and gather_sum_kernel writes each touched row of dW exactly once.  Here that
// list is the gradient's other half (optim_rows_abi.hpp): dW is never zeroed and never read outside the touched rows.
//   optim_rows_sqnorm_kernel        a wave per window of 64 sorted positions; the float64 sum of squares of every head's
//                                   row, one partial per workgroup in optim.hip's workspace;
//   optim_rows_adam_kernel<lazy>    the same windows; adam_element on the touched rows alone.  NOT the reference's
//                                   trajectory: dense Adam (model_mag.py:312) moves an untouched row while its moments decay;
//   optim_rows_adam_kernel<exact>   the table in chunks; adam_element on every element, with g = dW[row, h] for a touched
//                                   row and the literal 0.0f otherwise: bit for bit the dense kernel on a zero-filled dW.
// Heads and the row -> position search are optim_rows_layout.hpp's (HIP-free, held on the CPU by
// tests/native/optim_rows_check.cpp); AdamArgs, adam_element and the norm / coefficient out of the partials are
// optim_math.hpp's, the lines optim.hip runs.  No atomics, no host read; every argument travels by value.
#include "optim_math.hpp"
#include "optim_rows_layout.hpp"
#include "optim_rows_heads.hpp"
#include "optim_rows_abi.hpp"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kRowsChunk = 4096;                               // exact mode: table elements per unit of work
constexpr int kSlots = GP_OPTIM_WORKSPACE_BYTES / 8;           // optim.hip's f64 partials of the squared norm
constexpr int kMaxGrid = kSlots;
// Head rows of a window whose loads are in flight together.  16 (update) and 32 (norm) were tried at the bench shape of
// DESIGN §7t and changed neither kernel's time, at 320 VGPRs for the update; other shapes are unmeasured.
constexpr int kRowsAtOnce = 8;

static_assert(kSlots == kBlock * 4, "clip_coef reads four slots per thread");

struct RowsArgs {
    float* p; float* m; float* v; const float* dW;
    const long long* keys;
    long long n_sorted, V;
    int H;
};

__device__ __forceinline__ u64 window_heads(const RowsArgs& R, long long win, int lane, long long& key)
{
    const long long i = (win << 6) + lane;
    const bool in = i < R.n_sorted;
    key = in ? R.keys[i] : R.V;
    return __ballot(in && gp_optim_rows::is_head(R.keys, i, R.V));
}

__device__ __forceinline__ double sq(float x) { return (double)x * (double)x; }

__global__ __launch_bounds__(kBlock) void optim_rows_sqnorm_kernel(const RowsArgs R, double* __restrict__ partials, int accumulate)
{
    __shared__ double lds[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long n_win = gp_optim_rows::windows(R.n_sorted);
    double acc = 0.0;
    for (long long win = (long long)blockIdx.x * kWaves + wave; win < n_win; win += (long long)gridDim.x * kWaves) {   // wave-uniform
        long long key;
        u64 heads = window_heads(R, win, lane, key);
        while (heads) {
            long long rows[kRowsAtOnce];
            const int n = take_heads(heads, key, rows);
            for (int h0 = 0; h0 < R.H; h0 += 64) {
                const int h = h0 + lane;
                float g[kRowsAtOnce];
#pragma unroll
                for (int r = 0; r < kRowsAtOnce; ++r) g[r] = r < n && h < R.H ? R.dW[rows[r] * R.H + h] : 0.0f;
#pragma unroll
                for (int r = 0; r < kRowsAtOnce; ++r) acc += sq(g[r]);
            }
        }
    }
    const double s = block_sum<kWaves>(acc, lds);
    // slot blockIdx.x holds this workgroup's sum; a first launch also zeroes the slots no workgroup owns
    if (tid == 0) partials[blockIdx.x] = accumulate ? partials[blockIdx.x] + s : s;
    if (!accumulate)
        for (int i = gridDim.x + blockIdx.x * kBlock + tid; i < kSlots; i += gridDim.x * kBlock) partials[i] = 0.0;
}

template <bool kLazy, bool kDeviceSteps>
__global__ __launch_bounds__(kBlock) void optim_rows_adam_kernel(const RowsArgs R, const double* __restrict__ partials,
                                                                  float* __restrict__ norm_out, const AdamArgs a_in,
                                                                  const float* __restrict__ d_step_size,
                                                                  const float* __restrict__ d_rsqrt_bc2)
{
    __shared__ double lds[kWaves];
    __shared__ unsigned char s_touched[kLazy ? 1 : kRowsChunk + 1];
    AdamArgs a = a_in;
    if (kDeviceSteps) { a.step_size = *d_step_size; a.rsqrt_bc2 = *d_rsqrt_bc2; }
    const int tid = threadIdx.x;
    float norm;
    const float coef = clip_coef<kWaves>(partials, a.max_norm, lds, norm);
    if (norm_out && blockIdx.x == 0 && tid == 0) *norm_out = norm;
    const int H = R.H;

    if (kLazy) {
        const int lane = tid & 63, wave = tid >> 6;
        const long long n_win = gp_optim_rows::windows(R.n_sorted);
        for (long long win = (long long)blockIdx.x * kWaves + wave; win < n_win; win += (long long)gridDim.x * kWaves) {   // wave-uniform
            long long key;
            u64 heads = window_heads(R, win, lane, key);
            while (heads) {
                long long rows[kRowsAtOnce];
                const int n = take_heads(heads, key, rows);
                for (int h0 = 0; h0 < H; h0 += 64) {
                    const int h = h0 + lane;
                    if (h >= H) continue;
                    float g[kRowsAtOnce], p[kRowsAtOnce], m[kRowsAtOnce], v[kRowsAtOnce];
#pragma unroll
                    for (int r = 0; r < kRowsAtOnce; ++r) {
                        if (r < n) {
                            const long long at = rows[r] * H + h;
                            g[r] = R.dW[at]; p[r] = R.p[at]; m[r] = R.m[at]; v[r] = R.v[at];
                        }
                    }
#pragma unroll
                    for (int r = 0; r < kRowsAtOnce; ++r) {
                        if (r < n) {
                            const long long at = rows[r] * H + h;
                            adam_element(p[r], g[r], m[r], v[r], coef, a);
                            R.p[at] = p[r]; R.m[at] = m[r]; R.v[at] = v[r];
                        }
                    }
                }
            }
        }
        return;
    }

    // exact: chunk c is the elements [c * kRowsChunk, ...) of the flat table; they lie in at most kRowsChunk + 1 rows, whose
    // touched flags one search per row leaves in LDS (the key list is small and stays in L2)
    const long long total = R.V * H;
    const long long n_chunks = (total + kRowsChunk - 1) / kRowsChunk;
    const bool vec = (H & 3) == 0 && (((uintptr_t)R.dW | (uintptr_t)R.p | (uintptr_t)R.m | (uintptr_t)R.v) & 15) == 0;
    for (long long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const long long start = c * kRowsChunk;
        const long long left = total - start;
        const int n = left < kRowsChunk ? (int)left : kRowsChunk;
        const long long first_row = start / H;
        const unsigned off0 = (unsigned)(start - first_row * H);              // < H: the chunk's first element within its row
        const int n_rows = (int)((off0 + (unsigned)(n - 1)) / (unsigned)H) + 1;
        __syncthreads();                                                       // the chunk before has read its flags
        for (int r = tid; r < n_rows; r += kBlock) s_touched[r] = gp_optim_rows::touched(R.keys, R.n_sorted, first_row + r);
        __syncthreads();
        const float* g = R.dW + start;
        float* p = R.p + start;
        float* m = R.m + start;
        float* v = R.v + start;
        if (vec && n == kRowsChunk) {                                          // a whole chunk: every load is issued before the first use
            constexpr int kIter = kRowsChunk / (kBlock * 4);
            float4 g4[kIter], p4[kIter], m4[kIter], v4[kIter];
#pragma unroll
            for (int k = 0; k < kIter; ++k) {
                const int i = (k * kBlock + tid) * 4;                          // H % 4 == 0: the four lie in one row
                g4[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (s_touched[(off0 + (unsigned)i) / (unsigned)H]) g4[k] = *reinterpret_cast<const float4*>(g + i);
                p4[k] = *reinterpret_cast<const float4*>(p + i);
                m4[k] = *reinterpret_cast<const float4*>(m + i);
                v4[k] = *reinterpret_cast<const float4*>(v + i);
            }
#pragma unroll
            for (int k = 0; k < kIter; ++k) {
                const int i = (k * kBlock + tid) * 4;
                adam_element(p4[k].x, g4[k].x, m4[k].x, v4[k].x, coef, a);
                adam_element(p4[k].y, g4[k].y, m4[k].y, v4[k].y, coef, a);
                adam_element(p4[k].z, g4[k].z, m4[k].z, v4[k].z, coef, a);
                adam_element(p4[k].w, g4[k].w, m4[k].w, v4[k].w, coef, a);
                *reinterpret_cast<float4*>(p + i) = p4[k];
                *reinterpret_cast<float4*>(m + i) = m4[k];
                *reinterpret_cast<float4*>(v + i) = v4[k];
            }
        } else if (vec) {                                                      // the table's last chunk: n % 4 == 0 as H % 4 == 0
            for (int i = tid * 4; i < n; i += kBlock * 4) {
                float4 g4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (s_touched[(off0 + (unsigned)i) / (unsigned)H]) g4 = *reinterpret_cast<const float4*>(g + i);
                float4 p4 = *reinterpret_cast<const float4*>(p + i);
                float4 m4 = *reinterpret_cast<const float4*>(m + i);
                float4 v4 = *reinterpret_cast<const float4*>(v + i);
                adam_element(p4.x, g4.x, m4.x, v4.x, coef, a);
                adam_element(p4.y, g4.y, m4.y, v4.y, coef, a);
                adam_element(p4.z, g4.z, m4.z, v4.z, coef, a);
                adam_element(p4.w, g4.w, m4.w, v4.w, coef, a);
                *reinterpret_cast<float4*>(p + i) = p4;
                *reinterpret_cast<float4*>(m + i) = m4;
                *reinterpret_cast<float4*>(v + i) = v4;
            }
        } else {                                                               // H % 4 != 0 or an unaligned table: the same arithmetic
            for (int i = tid; i < n; i += kBlock) {
                float gi = 0.0f;
                if (s_touched[(off0 + (unsigned)i) / (unsigned)H]) gi = g[i];
                adam_element(p[i], gi, m[i], v[i], coef, a);
            }
        }
    }
}

int window_grid(long long n_sorted)
{
    const long long g = (gp_optim_rows::windows(n_sorted) + kWaves - 1) / kWaves;
    return (int)(g < 1 ? 1 : g < kMaxGrid ? g : kMaxGrid);
}

int rows_check(const char* where, const void* d_keys, int64_t n_sorted, int64_t n_vocab, int32_t dim)
{
    if (n_sorted < 0 || n_vocab < 1 || dim < 1) return fail(GP_ERR_INVALID_ARG, where, "n_sorted < 0, n_vocab < 1 or dim < 1");
    if (n_vocab > INT64_MAX / dim) return fail(GP_ERR_INVALID_ARG, where, "n_vocab * dim does not fit 63 bits");
    if (!d_keys) return fail(GP_ERR_NULL, where, "d_keys is NULL");
    return GP_OK;
}

// both entry points: kDeviceSteps says whether step_size / rsqrt_bc2 are the two values or the two device pointers
template <bool kDeviceSteps>
int clip_adam_rows(const char* where, int device, float* d_param, float* d_exp_avg, float* d_exp_avg_sq, const float* d_dW,
                   const int64_t* d_keys, int64_t n_sorted, int64_t n_vocab, int32_t dim, int mode, float max_norm, float lr,
                   double beta1, double beta2, float eps, float weight_decay, float step_size, float rsqrt_bc2,
                   const float* d_step_size, const float* d_rsqrt_bc2, void* d_workspace, float* d_norm_out, void* stream)
{
    if (mode != GP_OPTIM_ROWS_EXACT && mode != GP_OPTIM_ROWS_LAZY)
        return fail(GP_ERR_INVALID_ARG, where, "mode is neither GP_OPTIM_ROWS_EXACT nor GP_OPTIM_ROWS_LAZY");
    if (!std::isfinite(max_norm) || !std::isfinite(lr) || !std::isfinite(beta1) || !std::isfinite(beta2) || !std::isfinite(eps) ||
        !std::isfinite(weight_decay) || !std::isfinite(step_size) || !std::isfinite(rsqrt_bc2))
        return fail(GP_ERR_INVALID_ARG, where, "a hyper-parameter is not finite");
    if (mode == GP_OPTIM_ROWS_LAZY && weight_decay != 0.0f)
        return fail(GP_ERR_INVALID_ARG, where, "lazy mode takes weight_decay = 0: a decay on the touched rows alone is nobody's semantics");
    if (const int rc = rows_check(where, d_keys, n_sorted, n_vocab, dim)) return rc;
    if (!d_param || !d_exp_avg || !d_exp_avg_sq || !d_dW || !d_workspace || !d_norm_out)
        return fail(GP_ERR_NULL, where, "the table, its state, d_dW, the workspace or the norm output is NULL");
    if (kDeviceSteps && (!d_step_size || !d_rsqrt_bc2)) return fail(GP_ERR_NULL, where, "d_step_size or d_rsqrt_bc2 is NULL");
    if (mode == GP_OPTIM_ROWS_LAZY && n_sorted == 0) return GP_OK;               // nothing is touched
    if (const int rc = set_device(device, where)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const RowsArgs R = {d_param, d_exp_avg, d_exp_avg_sq, d_dW, (const long long*)d_keys, (long long)n_sorted, (long long)n_vocab, dim};
    const AdamArgs a = {max_norm, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, weight_decay,
                        step_size, rsqrt_bc2, 0};
    const double* partials = static_cast<const double*>(d_workspace);
    if (mode == GP_OPTIM_ROWS_LAZY) {
        hipLaunchKernelGGL((optim_rows_adam_kernel<true, kDeviceSteps>), dim3(window_grid(n_sorted)), dim3(kBlock), 0, s, R, partials,
                           d_norm_out, a, d_step_size, d_rsqrt_bc2);
    } else {
        const long long chunks = ((long long)n_vocab * dim + kRowsChunk - 1) / kRowsChunk;
        hipLaunchKernelGGL((optim_rows_adam_kernel<false, kDeviceSteps>), dim3((int)(chunks < kMaxGrid ? chunks : kMaxGrid)), dim3(kBlock),
                           0, s, R, partials, d_norm_out, a, d_step_size, d_rsqrt_bc2);
    }
    return launch_status("optim_rows_adam_kernel");
}

}  // namespace

extern "C" {

int gp_optim_rows_sqnorm(int device, const int64_t* d_keys, int64_t n_sorted, int64_t n_vocab, int32_t dim,
                         const float* d_dW, int accumulate, void* d_workspace, void* stream)
{
    const char* where = "gp_optim_rows_sqnorm";
    if (const int rc = rows_check(where, d_keys, n_sorted, n_vocab, dim)) return rc;
    if (!d_dW || !d_workspace) return fail(GP_ERR_NULL, where, "d_dW or the workspace is NULL");
    if (n_sorted == 0 && accumulate) return GP_OK;                               // nothing to add
    if (const int rc = set_device(device, where)) return rc;
    const RowsArgs R = {nullptr, nullptr, nullptr, d_dW, (const long long*)d_keys, (long long)n_sorted, (long long)n_vocab, dim};
    hipLaunchKernelGGL(optim_rows_sqnorm_kernel, dim3(window_grid(n_sorted)), dim3(kBlock), 0, (hipStream_t)stream, R,
                       static_cast<double*>(d_workspace), accumulate != 0);
    return launch_status("optim_rows_sqnorm_kernel");
}

int gp_clip_adam_rows(int device, float* d_param, float* d_exp_avg, float* d_exp_avg_sq, const float* d_dW,
                      const int64_t* d_keys, int64_t n_sorted, int64_t n_vocab, int32_t dim, int mode, float max_norm,
                      float lr, double beta1, double beta2, float eps, float weight_decay, float step_size, float rsqrt_bc2,
                      void* d_workspace, float* d_norm_out, void* stream)
{
    return clip_adam_rows<false>("gp_clip_adam_rows", device, d_param, d_exp_avg, d_exp_avg_sq, d_dW, d_keys, n_sorted, n_vocab, dim,
                                 mode, max_norm, lr, beta1, beta2, eps, weight_decay, step_size, rsqrt_bc2, nullptr, nullptr,
                                 d_workspace, d_norm_out, stream);
}

int gp_clip_adam_rows_dev(int device, float* d_param, float* d_exp_avg, float* d_exp_avg_sq, const float* d_dW,
                          const int64_t* d_keys, int64_t n_sorted, int64_t n_vocab, int32_t dim, int mode, float max_norm,
                          float lr, double beta1, double beta2, float eps, float weight_decay, const float* d_step_size,
                          const float* d_rsqrt_bc2, void* d_workspace, float* d_norm_out, void* stream)
{
    return clip_adam_rows<true>("gp_clip_adam_rows_dev", device, d_param, d_exp_avg, d_exp_avg_sq, d_dW, d_keys, n_sorted, n_vocab, dim,
                                mode, max_norm, lr, beta1, beta2, eps, weight_decay, 0.0f, 0.0f, d_step_size, d_rsqrt_bc2,
                                d_workspace, d_norm_out, stream);
}

}  // extern "C"
