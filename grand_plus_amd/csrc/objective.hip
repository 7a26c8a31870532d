// objective.hip -- GRAND+'s training objective after the MLP, fused.  Reference (model.py:123-139, 321-331;
// model_mag.py:125-142, 354-366), for S samples of logits z[s] [B x C], rows b < n_l labelled:
//
//     logp   = log_softmax(z[s])                                     (model.py:324)
//     L_sup  = (1/S) sum_s nll_loss(logp[s][:n_l], y)                 (model.py:326-327)
//     avg_p  = (1/S) sum_s exp(logp[s])                               (model.py:124-128)
//     q      = softmax(log(avg_p) / tem)   (sharp_p, detached)        (model.py:130)
//     L_con  = (1/S) sum_s mean_{avg_p.max(1) > conf} kl: sum_c -q logp / l2: sum_c (p - q)^2   (model.py:131-139)
//     loss   = L_sup + w * L_con                                      (model.py:329)
//
// Three kernels, no atomics, no host synchronisation:
//   grand_loss_rows_kernel    one wave per batch row: the row's S log-softmaxes, avg_p, q and its partials (sup, con,
//                             flags) into the caller's workspace;
//   grand_loss_reduce_kernel  one workgroup: the partials summed in a fixed order in fp64, the scalars written;
//   grand_loss_backward_kernel one wave per row: p and q recomputed, dz written from the device scalars.
// Sums over c and over s run in a fixed order (wave butterflies, then s ascending), so value and gradient are
// bitwise the same run to run.
#include "gp_common.hpp"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxS = 16;
constexpr int kMaxC = 4096;

enum { kFlagValid = 1, kFlagConf = 2, kFlagBad = 4, kFlagCorrect = 8 };

struct LossArgs {
    const float* z;                 // [S x B x C]
    int S; long long B; int C;
    const long long* labels;        // [n_l]
    long long n_l, ignore;
    float tem, conf;
    int kind;                       // GP_LOSS_KL / GP_LOSS_L2
    int logp_in;                    // z already holds log-probabilities
};

// Per-row state every pass needs: logp[s,c] = (z[s,c] - mx[s]) - ls[s] (torch's log_softmax order; 0 and 0 when z holds
// log-probabilities), the largest avg_p and q's normaliser: q_c = exp(t_c - tmax) / tsum, t_c = log(avg_p_c) / tem.
struct RowStats {
    float* mx; float* ls;           // [kMaxS] each, in the wave's own LDS slots (indexed by a runtime s)
    float amax, tmax, tsum;
};

struct RowView {
    const float* z; size_t s_stride; int S; int C; float tem;

    __device__ __forceinline__ float logp(const RowStats& r, int s, int c) const
    {
        return (z[s * s_stride + c] - r.mx[s]) - r.ls[s];
    }
    // avg_p_c as the reference forms it ((0 + p_0) + p_1 ...) / S, and t_c from the log domain:
    // log avg_p = m + log(sum_s exp(logp_s - m)) - log S, m = max_s logp_s
    __device__ __forceinline__ void avg(const RowStats& r, int c, float& avg_p, float& t) const
    {
        float psum = 0.0f, m = -INFINITY;
#pragma unroll
        for (int s = 0; s < kMaxS; ++s) {
            if (s >= S) break;
            const float lp = logp(r, s, c);
            psum += expf(lp);
            m = fmaxf(m, lp);
        }
        float e = 0.0f;
#pragma unroll
        for (int s = 0; s < kMaxS; ++s) {
            if (s >= S) break;
            e += expf(logp(r, s, c) - m);
        }
        avg_p = psum / (float)S;
        t = (m + logf(e) - logf((float)S)) / tem;
    }
};

__device__ void row_stats(const RowView& v, int logp_in, int lane, RowStats& r)
{
    for (int s = 0; s < v.S; ++s) {                   // every lane stores the same value and reads only after its own store
        r.mx[s] = 0.0f; r.ls[s] = 0.0f;
        if (logp_in) continue;
        const float* zs = v.z + s * v.s_stride;
        float m = -INFINITY;
        for (int c = lane; c < v.C; c += 64) m = fmaxf(m, zs[c]);
        m = wave_max(m);
        float e = 0.0f;
        for (int c = lane; c < v.C; c += 64) e += expf(zs[c] - m);
        r.mx[s] = m;
        r.ls[s] = logf(wave_sum(e));
    }
    float amax = -INFINITY, tmax = -INFINITY;
    for (int c = lane; c < v.C; c += 64) {
        float a, t;
        v.avg(r, c, a, t);
        amax = fmaxf(amax, a);
        tmax = fmaxf(tmax, t);
    }
    r.amax = wave_max(amax);
    r.tmax = wave_max(tmax);
    float ts = 0.0f;
    for (int c = lane; c < v.C; c += 64) {
        float a, t;
        v.avg(r, c, a, t);
        ts += expf(t - r.tmax);
    }
    r.tsum = wave_sum(ts);
}

// Which set row b belongs to: supervised (valid label), consistency (confident unlabelled row), or neither.
__device__ __forceinline__ void row_sets(const LossArgs& a, long long b, const RowStats& r, long long& y, bool& valid, bool& bad, bool& conf)
{
    y = -1; valid = bad = conf = false;
    if (b < a.n_l) {
        y = a.labels[b];
        if (y != a.ignore) {
            if (y >= 0 && y < a.C) valid = true;
            else bad = true;                          // never used as an index; counted
        }
    } else {
        conf = r.amax > a.conf;                       // strict, model.py:134/136
    }
}

__global__ void __launch_bounds__(kBlock)
grand_loss_rows_kernel(LossArgs a, double* __restrict__ part, int* __restrict__ flags)
{
    const int lane = threadIdx.x & 63;
    const long long n_waves = (long long)gridDim.x * kWaves;
    const size_t s_stride = (size_t)a.B * a.C;
    __shared__ float s_ml[kWaves][2][kMaxS];
    for (long long b = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6); b < a.B; b += n_waves) {   // wave-uniform
        const RowView v = {a.z + (size_t)b * a.C, s_stride, a.S, a.C, a.tem};
        RowStats r;
        r.mx = s_ml[threadIdx.x >> 6][0]; r.ls = s_ml[threadIdx.x >> 6][1];
        row_stats(v, a.logp_in, lane, r);
        long long y; bool valid, bad, conf;
        row_sets(a, b, r, y, valid, bad, conf);
        double sup = 0.0, con = 0.0;
        int fl = (valid ? kFlagValid : 0) | (bad ? kFlagBad : 0) | (conf ? kFlagConf : 0);
        if (valid) {
#pragma unroll
            for (int s = 0; s < kMaxS; ++s) {
                if (s >= a.S) break;
                sup += (double)(-v.logp(r, s, (int)y));                          // nll_loss, model.py:326
            }
            // accuracy of the last sample (model.py:333): first index of the row's largest logit
            const float* zl = v.z + (size_t)(a.S - 1) * s_stride;
            float best = -INFINITY; int arg = 0x7FFFFFFF;
            for (int c = lane; c < a.C; c += 64) if (zl[c] > best) { best = zl[c]; arg = c; }
            for (int o = 32; o > 0; o >>= 1) {
                const float ob = __shfl_xor(best, o); const int oa = __shfl_xor(arg, o);
                if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
            }
            if (arg == y) fl |= kFlagCorrect;
        }
        if (conf) {
            float acc[kMaxS];
#pragma unroll
            for (int s = 0; s < kMaxS; ++s) acc[s] = 0.0f;
            for (int c = lane; c < a.C; c += 64) {
                float av, t;
                v.avg(r, c, av, t);
                const float q = expf(t - r.tmax) / r.tsum;
#pragma unroll
                for (int s = 0; s < kMaxS; ++s) {
                    if (s >= a.S) break;
                    const float lp = v.logp(r, s, c);
                    if (a.kind == GP_LOSS_KL) acc[s] += -q * lp;
                    else { const float d = expf(lp) - q; acc[s] += d * d; }
                }
            }
#pragma unroll
            for (int s = 0; s < kMaxS; ++s) {
                if (s >= a.S) break;
                con += (double)wave_sum(acc[s]);
            }
        }
        if (lane == 0) { part[2 * b] = sup; part[2 * b + 1] = con; flags[b] = fl; }
    }
}

// One workgroup: thread t sums rows t, t + kBlock, ... in order, then a fixed tree.  out = {loss, L_sup, L_con},
// counts = {n_conf, n_valid, n_correct, n_bad}.  A mean over an empty set is 0/0 = NaN, as torch.mean of an empty tensor.
__global__ void __launch_bounds__(kBlock)
grand_loss_reduce_kernel(const double* __restrict__ part, const int* __restrict__ flags, long long B, int S, float weight,
                         float* __restrict__ out, int* __restrict__ counts)
{
    __shared__ double s_sup[kBlock], s_con[kBlock];
    __shared__ int s_cnt[4][kBlock];
    double sup = 0.0, con = 0.0;
    int n_conf = 0, n_valid = 0, n_correct = 0, n_bad = 0;
    for (long long b = threadIdx.x; b < B; b += kBlock) {
        sup += part[2 * b]; con += part[2 * b + 1];
        const int f = flags[b];
        n_conf += (f & kFlagConf) != 0; n_valid += (f & kFlagValid) != 0;
        n_correct += (f & kFlagCorrect) != 0; n_bad += (f & kFlagBad) != 0;
    }
    const int t = threadIdx.x;
    s_sup[t] = sup; s_con[t] = con;
    s_cnt[0][t] = n_conf; s_cnt[1][t] = n_valid; s_cnt[2][t] = n_correct; s_cnt[3][t] = n_bad;
    __syncthreads();
    for (int h = kBlock / 2; h > 0; h >>= 1) {
        if (t < h) {
            s_sup[t] += s_sup[t + h]; s_con[t] += s_con[t + h];
            for (int i = 0; i < 4; ++i) s_cnt[i][t] += s_cnt[i][t + h];
        }
        __syncthreads();
    }
    if (t == 0) {
        const double l_sup = s_sup[0] / (double)s_cnt[1][0] / (double)S;
        const double l_con = s_con[0] / (double)s_cnt[0][0] / (double)S;
        out[0] = (float)(l_sup + (double)weight * l_con);
        out[1] = (float)l_sup;
        out[2] = (float)l_con;
        for (int i = 0; i < 4; ++i) counts[i] = s_cnt[i][0];
    }
}

// dz from the device scalars: c_sup = (dloss + dL_sup) / (S n_valid), c_con = (w dloss + dL_con) / (S n_conf).
//   supervised   z: c_sup (p - onehot(y))                 logp: -c_sup onehot(y)
//   kl           z: c_con (p sum q - q)                   logp: -c_con q
//   l2           z: p (g - <g, p>), g = 2 c_con (p - q)   logp: g p
// Rows outside both sets get zeros.
__global__ void __launch_bounds__(kBlock)
grand_loss_backward_kernel(LossArgs a, float weight, const float* __restrict__ g_loss, const float* __restrict__ g_sup,
                           const float* __restrict__ g_con, const int* __restrict__ counts, float* __restrict__ dz)
{
    const int lane = threadIdx.x & 63;
    const long long n_waves = (long long)gridDim.x * kWaves;
    const size_t s_stride = (size_t)a.B * a.C;
    const float gl = *g_loss;
    const float c_sup = (gl + (g_sup ? *g_sup : 0.0f)) / ((float)a.S * (float)counts[1]);
    const float c_con = (weight * gl + (g_con ? *g_con : 0.0f)) / ((float)a.S * (float)counts[0]);
    __shared__ float s_ml[kWaves][2][kMaxS];
    for (long long b = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6); b < a.B; b += n_waves) {
        const RowView v = {a.z + (size_t)b * a.C, s_stride, a.S, a.C, a.tem};
        float* dzr = dz + (size_t)b * a.C;
        RowStats r;
        r.mx = s_ml[threadIdx.x >> 6][0]; r.ls = s_ml[threadIdx.x >> 6][1];
        row_stats(v, a.logp_in, lane, r);
        long long y; bool valid, bad, conf;
        row_sets(a, b, r, y, valid, bad, conf);
        if (valid) {
            for (int s = 0; s < a.S; ++s)
                for (int c = lane; c < a.C; c += 64) {
                    const float oh = c == y ? 1.0f : 0.0f;
                    dzr[s * s_stride + c] = a.logp_in ? -c_sup * oh : c_sup * (expf(v.logp(r, s, c)) - oh);
                }
        } else if (conf) {
            float qs = 0.0f;
            for (int c = lane; c < a.C; c += 64) {
                float av, t;
                v.avg(r, c, av, t);
                qs += expf(t - r.tmax) / r.tsum;
            }
            qs = wave_sum(qs);
            for (int s = 0; s < a.S; ++s) {
                float dot = 0.0f;
                if (a.kind == GP_LOSS_L2 && !a.logp_in) {
                    for (int c = lane; c < a.C; c += 64) {
                        float av, t;
                        v.avg(r, c, av, t);
                        const float q = expf(t - r.tmax) / r.tsum, p = expf(v.logp(r, s, c));
                        dot += (2.0f * c_con * (p - q)) * p;
                    }
                    dot = wave_sum(dot);
                }
                for (int c = lane; c < a.C; c += 64) {
                    float av, t;
                    v.avg(r, c, av, t);
                    const float q = expf(t - r.tmax) / r.tsum, p = expf(v.logp(r, s, c));
                    float d;
                    if (a.kind == GP_LOSS_KL) d = a.logp_in ? -c_con * q : c_con * (p * qs - q);
                    else {
                        const float g = 2.0f * c_con * (p - q);
                        d = a.logp_in ? g * p : p * (g - dot);
                    }
                    dzr[s * s_stride + c] = d;
                }
            }
        } else {
            for (int s = 0; s < a.S; ++s)
                for (int c = lane; c < a.C; c += 64) dzr[s * s_stride + c] = 0.0f;
        }
    }
}

int check_loss_args(const char* where, const float* d_z, int32_t S, int64_t B, int32_t C, const int64_t* d_labels, int64_t n_l,
                    float tem, int kind)
{
    if (S < 1 || S > kMaxS || B < 0 || C < 1 || C > kMaxC || n_l < 0 || n_l > B || !(tem > 0.0f) ||
        (kind != GP_LOSS_KL && kind != GP_LOSS_L2))
        return fail(GP_ERR_INVALID_ARG, where,
                              "n_samples outside [1, 16], n_classes outside [1, 4096], n_rows < 0, n_labeled outside [0, n_rows], "
                              "tem <= 0 or unknown kind");
    if ((B > 0 && !d_z) || (n_l > 0 && !d_labels)) return fail(GP_ERR_NULL, where, "a device pointer is NULL");
    return GP_OK;
}

}  // namespace

extern "C" {

int gp_grand_loss(int device, const float* d_z, int32_t n_samples, int64_t n_rows, int32_t n_classes,
                  const int64_t* d_labels, int64_t n_labeled, int64_t ignore_index, float weight, float tem, float conf,
                  int kind, int inputs_are_log_probs, void* d_workspace, float* d_out, int32_t* d_counts, void* stream)
{
    const char* where = "gp_grand_loss";
    if (const int rc = check_loss_args(where, d_z, n_samples, n_rows, n_classes, d_labels, n_labeled, tem, kind)) return rc;
    if (!d_out || !d_counts || (n_rows > 0 && !d_workspace)) return fail(GP_ERR_NULL, where, "a device pointer is NULL");
    if (const int rc = set_device(device, where)) return rc;
    hipStream_t s = (hipStream_t)stream;
    double* part = static_cast<double*>(d_workspace);
    int* flags = reinterpret_cast<int*>(part + 2 * n_rows);
    const LossArgs a = {d_z, n_samples, (long long)n_rows, n_classes, (const long long*)d_labels, (long long)n_labeled,
                        (long long)ignore_index, tem, conf, kind, inputs_are_log_probs != 0};
    if (n_rows > 0) {
        hipLaunchKernelGGL(grand_loss_rows_kernel, dim3(row_grid(n_rows, kWaves)), dim3(kBlock), 0, s, a, part, flags);
        if (const int rc = launch_status("grand_loss_rows_kernel")) return rc;
    }
    hipLaunchKernelGGL(grand_loss_reduce_kernel, dim3(1), dim3(kBlock), 0, s, part, flags, (long long)n_rows, n_samples, weight,
                       d_out, (int*)d_counts);
    return launch_status("grand_loss_reduce_kernel");
}

int gp_grand_loss_backward(int device, const float* d_z, int32_t n_samples, int64_t n_rows, int32_t n_classes,
                           const int64_t* d_labels, int64_t n_labeled, int64_t ignore_index, float weight, float tem, float conf,
                           int kind, int inputs_are_log_probs, const float* d_grad_loss, const float* d_grad_sup,
                           const float* d_grad_con, const int32_t* d_counts, float* d_grad_z, void* stream)
{
    const char* where = "gp_grand_loss_backward";
    if (const int rc = check_loss_args(where, d_z, n_samples, n_rows, n_classes, d_labels, n_labeled, tem, kind)) return rc;
    if (!d_grad_loss || !d_counts || (n_rows > 0 && !d_grad_z)) return fail(GP_ERR_NULL, where, "a device pointer is NULL");
    if (n_rows == 0) return GP_OK;
    if (const int rc = set_device(device, where)) return rc;
    const LossArgs a = {d_z, n_samples, (long long)n_rows, n_classes, (const long long*)d_labels, (long long)n_labeled,
                        (long long)ignore_index, tem, conf, kind, inputs_are_log_probs != 0};
    hipLaunchKernelGGL(grand_loss_backward_kernel, dim3(row_grid(n_rows, kWaves)), dim3(kBlock), 0, (hipStream_t)stream, a, weight,
                       d_grad_loss, d_grad_sup, d_grad_con, (const int*)d_counts, d_grad_z);
    return launch_status("grand_loss_backward_kernel");
}

}  // extern "C"
