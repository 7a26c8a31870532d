// optim.hip -- the end of a GRAND+ training step, fused.  Reference (model.py:116-120, 333-334; same in
// model_mag.py):
//
//     grad_norm = clip_grad_norm(model.parameters(), args.clip_norm)   # one 2-norm over every gradient; scaled when > 0
//     optimizer.step()                                                  # torch.optim.Adam, weight_decay as L2
//
// The models train 3-9 small parameter tensors, so the cost is launches, not bytes.  Two kernels, no atomics, no host
// synchronisation; the tensors of a call travel BY VALUE in the kernel arguments (grad pointers change every step, a
// device-side table would need an upload per step):
//   optim_sqnorm_kernel     work is cut into chunks of kChunk elements of one tensor; a workgroup takes chunks grid-stride,
//                           sums the squares of the gradients in float64 (an fp32 square is exact there) and leaves one
//                           partial per workgroup in one of kSlots workspace slots (the rest are zeroed);
//   optim_clip_adam_kernel  every workgroup sums the kSlots partials in index order with the same fixed tree, so all hold
//                           the same bits; norm, clip coefficient, then the Adam update (or, with GP_OPTIM_CLIP_ONLY,
//                           grad * coef written back) over its chunks.  A template on where step_size and rsqrt_bc2 come
//                           from: the kernel arguments (gp_clip_adam_step), or two device floats of a gp_step_state
//                           (gp_clip_adam_step_dev), read once per thread before the same arithmetic.
// A chunk whose four pointers are 16-byte aligned moves as float4; any other takes a scalar path with the same
// per-element arithmetic (-ffp-contract=off: no fused multiply-add), so an element's result never depends on where it lies.
// AdamArgs, adam_element and the norm / coefficient out of the partials are optim_math.hpp's, shared with optim_rows.hip.
#include "optim_math.hpp"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kChunk = 4096;                                   // elements of one tensor per unit of work
constexpr int kSlots = GP_OPTIM_WORKSPACE_BYTES / 8;           // f64 partials of the squared norm
constexpr int kMaxGrid = kSlots;

static_assert(kSlots == kBlock * 4, "the partial sum reads four slots per thread");

struct OptimEntry {
    float* p; const float* g; float* m; float* v;
    long long n;                 // elements
    long long chunk_end;         // chunks of this and every earlier entry of the table
};

struct OptimTable {
    OptimEntry e[GP_OPTIM_MAX_TENSORS];
    int n;
    int pad;
};

static_assert(sizeof(OptimTable) <= 2048, "the table travels in the kernel arguments (4 KB)");

// the entry of chunk c: the first whose chunk_end exceeds c (entries of 0 elements are never found)
__device__ __forceinline__ int entry_of(const OptimTable& tab, long long c)
{
    int lo = 0, hi = tab.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (c < tab.e[mid].chunk_end) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ double sq(float x) { return (double)x * (double)x; }

__global__ __launch_bounds__(kBlock) void optim_sqnorm_kernel(const OptimTable tab, double* __restrict__ partials, int accumulate)
{
    __shared__ double lds[kWaves];
    const int tid = threadIdx.x;
    const long long total = tab.n > 0 ? tab.e[tab.n - 1].chunk_end : 0;
    double acc = 0.0;
    for (long long c = blockIdx.x; c < total; c += gridDim.x) {
        const int t = entry_of(tab, c);
        const long long first = t > 0 ? tab.e[t - 1].chunk_end : 0;
        const long long start = (c - first) * kChunk;
        const long long left = tab.e[t].n - start;
        const int n = left < kChunk ? (int)left : kChunk;
        const float* __restrict__ g = tab.e[t].g + start;
        if (((uintptr_t)g & 15) == 0) {
            const int n4 = n & ~3;
#pragma unroll 4
            for (int i = tid * 4; i < n4; i += kBlock * 4) {
                const float4 x = *reinterpret_cast<const float4*>(g + i);
                acc += sq(x.x); acc += sq(x.y); acc += sq(x.z); acc += sq(x.w);
            }
            if (n4 + tid < n) acc += sq(g[n4 + tid]);
        } else {
            for (int i = tid; i < n; i += kBlock) acc += sq(g[i]);
        }
    }
    const double s = block_sum<kWaves>(acc, lds);
    // slot blockIdx.x holds this workgroup's sum; a first launch also zeroes the slots no workgroup owns
    if (tid == 0) partials[blockIdx.x] = accumulate ? partials[blockIdx.x] + s : s;
    if (!accumulate)
        for (int i = gridDim.x + blockIdx.x * kBlock + tid; i < kSlots; i += gridDim.x * kBlock) partials[i] = 0.0;
}

template <bool kDeviceSteps>
__global__ __launch_bounds__(kBlock) void optim_clip_adam_kernel(const OptimTable tab, const double* __restrict__ partials,
                                                                  float* __restrict__ norm_out, long long n_chunks, const AdamArgs a_in,
                                                                  const float* __restrict__ d_step_size,
                                                                  const float* __restrict__ d_rsqrt_bc2)
{
    __shared__ double lds[kWaves];
    AdamArgs a = a_in;
    if (kDeviceSteps) { a.step_size = *d_step_size; a.rsqrt_bc2 = *d_rsqrt_bc2; }
    const int tid = threadIdx.x;
    float norm;
    const float coef = clip_coef<kWaves>(partials, a.max_norm, lds, norm);
    if (norm_out && blockIdx.x == 0 && tid == 0) *norm_out = norm;

    for (long long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int t = entry_of(tab, c);
        const long long first = t > 0 ? tab.e[t - 1].chunk_end : 0;
        const long long start = (c - first) * kChunk;
        const long long left = tab.e[t].n - start;
        const int n = left < kChunk ? (int)left : kChunk;
        const float* g = tab.e[t].g + start;
        if (a.clip_only) {
            float* go = const_cast<float*>(g);                // clip-only: the gradient is the output
            if (((uintptr_t)g & 15) == 0) {
                const int n4 = n & ~3;
                for (int i = tid * 4; i < n4; i += kBlock * 4) {
                    float4 x = *reinterpret_cast<const float4*>(g + i);
                    x.x *= coef; x.y *= coef; x.z *= coef; x.w *= coef;
                    *reinterpret_cast<float4*>(go + i) = x;
                }
                if (n4 + tid < n) go[n4 + tid] = g[n4 + tid] * coef;
            } else {
                for (int i = tid; i < n; i += kBlock) go[i] = g[i] * coef;
            }
            continue;
        }
        float* p = tab.e[t].p + start;
        float* m = tab.e[t].m + start;
        float* v = tab.e[t].v + start;
        const bool aligned = (((uintptr_t)g | (uintptr_t)p | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
        if (aligned && n == kChunk) {                         // a whole chunk: every load is issued before the first use
            constexpr int kIter = kChunk / (kBlock * 4);
            float4 g4[kIter], p4[kIter], m4[kIter], v4[kIter];
#pragma unroll
            for (int k = 0; k < kIter; ++k) {
                const int i = (k * kBlock + tid) * 4;
                g4[k] = *reinterpret_cast<const float4*>(g + i);
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
        } else if (aligned) {
            const int n4 = n & ~3;
            for (int i = tid * 4; i < n4; i += kBlock * 4) {
                const float4 g4 = *reinterpret_cast<const float4*>(g + i);
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
            if (n4 + tid < n) adam_element(p[n4 + tid], g[n4 + tid], m[n4 + tid], v[n4 + tid], coef, a);
        } else {
            for (int i = tid; i < n; i += kBlock) adam_element(p[i], g[i], m[i], v[i], coef, a);
        }
    }
}

int grid_of(long long chunks) { return (int)(chunks < 1 ? 1 : chunks < kMaxGrid ? chunks : kMaxGrid); }

// entries [first, first + count) of the caller's array as one by-value table
long long fill_table(OptimTable& tab, const gp_optim_tensor* tensors, int first, int count)
{
    long long chunks = 0;
    for (int i = 0; i < count; ++i) {
        const gp_optim_tensor& t = tensors[first + i];
        chunks += (t.numel + kChunk - 1) / kChunk;
        tab.e[i] = {t.param, t.grad, t.exp_avg, t.exp_avg_sq, (long long)t.numel, chunks};
    }
    tab.n = count;
    tab.pad = 0;
    return chunks;
}

// both entry points: kDeviceSteps says whether step_size / rsqrt_bc2 are the two values or the two device pointers
template <bool kDeviceSteps>
int clip_adam_step(const char* where, int device, const gp_optim_tensor* tensors, int32_t n_tensors, int flags,
                   float max_norm, float lr, double beta1, double beta2, float eps, float weight_decay,
                   float step_size, float rsqrt_bc2, const float* d_step_size, const float* d_rsqrt_bc2,
                   void* d_workspace, float* d_norm_out, void* stream)
{
    const int known = GP_OPTIM_CLIP_ONLY | GP_OPTIM_NORM_ONLY | GP_OPTIM_NORM_READY;
    const bool clip_only = flags & GP_OPTIM_CLIP_ONLY, norm_only = flags & GP_OPTIM_NORM_ONLY, norm_ready = flags & GP_OPTIM_NORM_READY;
    if (n_tensors < 0 || (flags & ~known) || (norm_only && norm_ready))
        return fail(GP_ERR_INVALID_ARG, where, "n_tensors < 0, an unknown flag, or GP_OPTIM_NORM_ONLY together with GP_OPTIM_NORM_READY");
    if (!std::isfinite(max_norm) || !std::isfinite(lr) || !std::isfinite(beta1) || !std::isfinite(beta2) || !std::isfinite(eps) ||
        !std::isfinite(weight_decay) || !std::isfinite(step_size) || !std::isfinite(rsqrt_bc2))
        return fail(GP_ERR_INVALID_ARG, where, "a hyper-parameter is not finite");
    if ((n_tensors > 0 && !tensors) || !d_workspace || (!norm_only && !d_norm_out))
        return fail(GP_ERR_NULL, where, "the tensor table, the workspace or the norm output is NULL");
    if (kDeviceSteps && !norm_only && (!d_step_size || !d_rsqrt_bc2))
        return fail(GP_ERR_NULL, where, "d_step_size or d_rsqrt_bc2 is NULL");
    for (int i = 0; i < n_tensors; ++i) {
        const gp_optim_tensor& t = tensors[i];
        if (t.numel < 0) return fail(GP_ERR_INVALID_ARG, where, "a tensor has a negative element count");
        if (t.numel > 0 && (!t.grad || (!clip_only && !norm_only && (!t.param || !t.exp_avg || !t.exp_avg_sq))))
            return fail(GP_ERR_NULL, where, "a tensor pointer is NULL");
    }
    if (const int rc = set_device(device, where)) return rc;
    hipStream_t s = (hipStream_t)stream;
    double* partials = static_cast<double*>(d_workspace);
    const int n_groups = n_tensors > 0 ? (n_tensors + GP_OPTIM_MAX_TENSORS - 1) / GP_OPTIM_MAX_TENSORS : 1;
    OptimTable tab = {};

    if (!norm_ready) {
        // the first launch owns the most slots, so that every later group adds into slots that were written
        int slots = 1;
        for (int g = 0; g < n_groups; ++g) {
            const int first = g * GP_OPTIM_MAX_TENSORS;
            const int count = n_tensors - first < GP_OPTIM_MAX_TENSORS ? n_tensors - first : GP_OPTIM_MAX_TENSORS;
            const int grid = grid_of(fill_table(tab, tensors, first, count));
            if (grid > slots) slots = grid;
        }
        for (int g = 0; g < n_groups; ++g) {
            const int first = g * GP_OPTIM_MAX_TENSORS;
            const int count = n_tensors - first < GP_OPTIM_MAX_TENSORS ? n_tensors - first : GP_OPTIM_MAX_TENSORS;
            const long long chunks = fill_table(tab, tensors, first, count);
            if (g > 0 && chunks == 0) continue;
            hipLaunchKernelGGL(optim_sqnorm_kernel, dim3(g == 0 ? slots : grid_of(chunks)), dim3(kBlock), 0, s, tab, partials, g > 0);
            if (const int rc = launch_status("optim_sqnorm_kernel")) return rc;
        }
    }
    if (norm_only) return GP_OK;

    const AdamArgs a = {max_norm, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, weight_decay,
                        step_size, rsqrt_bc2, clip_only};
    const bool writes = !(clip_only && !(max_norm > 0.0f));       // clip-only with clipping off: the norm alone
    for (int g = 0; g < n_groups; ++g) {
        const int first = g * GP_OPTIM_MAX_TENSORS;
        const int count = n_tensors - first < GP_OPTIM_MAX_TENSORS ? n_tensors - first : GP_OPTIM_MAX_TENSORS;
        const long long chunks = fill_table(tab, tensors, first, writes ? count : 0);
        if (g > 0 && chunks == 0) continue;
        hipLaunchKernelGGL(optim_clip_adam_kernel<kDeviceSteps>, dim3(grid_of(chunks)), dim3(kBlock), 0, s, tab,
                           (const double*)partials, g == 0 ? d_norm_out : (float*)nullptr, chunks, a, d_step_size, d_rsqrt_bc2);
        if (const int rc = launch_status("optim_clip_adam_kernel")) return rc;
    }
    return GP_OK;
}

}  // namespace

extern "C" {

int gp_clip_adam_step(int device, const gp_optim_tensor* tensors, int32_t n_tensors, int flags,
                      float max_norm, float lr, double beta1, double beta2, float eps, float weight_decay,
                      float step_size, float rsqrt_bc2, void* d_workspace, float* d_norm_out, void* stream)
{
    return clip_adam_step<false>("gp_clip_adam_step", device, tensors, n_tensors, flags, max_norm, lr, beta1, beta2, eps,
                                 weight_decay, step_size, rsqrt_bc2, nullptr, nullptr, d_workspace, d_norm_out, stream);
}

int gp_clip_adam_step_dev(int device, const gp_optim_tensor* tensors, int32_t n_tensors, int flags,
                          float max_norm, float lr, double beta1, double beta2, float eps, float weight_decay,
                          const float* d_step_size, const float* d_rsqrt_bc2, void* d_workspace, float* d_norm_out, void* stream)
{
    return clip_adam_step<true>("gp_clip_adam_step_dev", device, tensors, n_tensors, flags, max_norm, lr, beta1, beta2, eps,
                                weight_decay, 0.0f, 0.0f, d_step_size, d_rsqrt_bc2, d_workspace, d_norm_out, stream);
}

}  // extern "C"
