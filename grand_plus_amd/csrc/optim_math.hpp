// optim_math.hpp -- the element arithmetic of the clip + Adam step, stated once for optim.hip (every
// element of every tensor) and optim_rows.hip (the embedding table by its touched rows): the hyper-parameters
// as the kernels take them, the update of one element, and how the norm and the clip coefficient come out of the
// workspace's float64 partials.  Everything has internal linkage, as in gp_common.hpp.
#pragma once

#include "gp_common.hpp"

#include <cmath>

namespace {

struct AdamArgs {
    float max_norm, beta1, beta2, one_minus_beta1, one_minus_beta2, eps, weight_decay, step_size, rsqrt_bc2;
    int clip_only;
};

__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, float coef, const AdamArgs& a)
{
    g = g * coef + a.weight_decay * p;
    m = a.beta1 * m + a.one_minus_beta1 * g;
    v = a.beta2 * v + a.one_minus_beta2 * g * g;
    p -= a.step_size * (m / (sqrtf(v) * a.rsqrt_bc2 + a.eps));
}

// The clip coefficient, and the norm it comes from, out of the NW * 256 float64 partials of the squared norm.  Every
// workgroup (NW waves, four slots per thread) sums them in index order with the same fixed tree, so all hold the same bits.
template <int NW>
__device__ __forceinline__ float clip_coef(const double* __restrict__ partials, float max_norm, double* lds, float& norm)
{
    const double* q = partials + threadIdx.x * 4;
    const double sum = block_sum<NW>(((q[0] + q[1]) + q[2]) + q[3], lds);
    norm = (float)sqrt(sum);
    float coef = 1.0f;
    if (max_norm > 0.0f) {
        const float c = max_norm / (norm + 1e-6f);
        coef = c >= 1.0f ? 1.0f : c;                          // torch.clamp(max=1): a NaN stays a NaN
    }
    return coef;
}

}  // namespace
