// mlp_eval.hpp -- the arithmetic of the MLP in eval mode, defined once for mlp.hip (§7f's eval mode), mlp_infer.hip (§7j)
// and mlp_chain.hip (§7l).  The three promise each other's bits; they keep the promise by calling the same lines.
//
// Arithmetic contract of an eval block  y = a W^T + b,  a = BN_running( node_norm( relu?(x) ) )  (-ffp-contract=off):
//     a[m,k] = (relu?(x[m,k]) * r_m) * mul_k + add_k                           eval_prologue; each factor only if its flag is set
//     acc = +0;  for k = 0 ... F-1 ascending: acc = fma(a[m,k], W[n,k], acc);  y[m,n] = acc + b[n]
// one chain per output whatever the tile, M or N (the k tail up to the next multiple of 16 adds fma(0, 0, acc)).
//     r_m   = 1 / (1e-12 + sqrt(ss)),  ss: lane l of a wave sums relu?(x[m,k])^2 over k = l, l + 64, ... ascending,
//             then the wave_sum butterfly                                      row_inv_norm
//     mul_k = gamma_k * is_k,  add_k = beta_k - mean_k * (gamma_k * is_k),  is_k = 1 / sqrt(var_k + eps)      bn_affine
// relu keeps a NaN in mlp_infer.hip and mlp_chain.hip (relu_nan, torch's rule), so a NaN in input row m makes output row m
// NaN through every layer; mlp.hip's fmaxf turns it into 0.  On every other value the two agree bit for bit.
// Output row m depends on input row m and the parameters only; no atomics.
//
// Everything has internal linkage, as in gp_common.hpp; a unit that launches neither kernel below (mlp.hip) still
// carries their 231 instructions in its code object.
#pragma once

#include "gp_common.hpp"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kBlock = 256;
constexpr int kBK = 16;               // reduction depth of an LDS row (one stage of the eval GEMMs)
constexpr int kStride = kBK + 4;      // floats between the LDS rows of a stage
constexpr long long kMaxGrid = 1ll << 22;   // workgroups per launch (grid.x * 256 threads stays below 2^32)

inline long long cdiv(long long a, long long b) { return (a + b - 1) / b; }

// relu that keeps a NaN (fmaxf alone gives 0, and a bad input row would come out finite after the first hidden layer);
// for every other value it is fmaxf(v, 0), bit for bit
__device__ __forceinline__ float relu_nan(float v) { return v != v ? v : fmaxf(v, 0.0f); }

// where k (0 ... 15) of an LDS row is stored, so that the k of one lane, in step order, are contiguous: a lane of
// 32x32x2 holds k = 2 s + (lane >> 5) of step s, a lane of 16x16x4 k = 4 s + (lane >> 4)
__device__ __forceinline__ int kperm32(int k) { return (k & 1) * 8 + (k >> 1); }
__device__ __forceinline__ int kperm16(int k) { return (k & 3) * 4 + (k >> 2); }

// PER consecutive k of one row from global memory: float4 where VEC says the pointers and K allow it
template <int PER, bool VEC>
__device__ __forceinline__ void load_row(const float* __restrict__ p, bool row_ok, int k, int K, float* v)
{
    if (VEC) {
#pragma unroll
        for (int q = 0; q < PER / 4; ++q) {
            float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (row_ok && k + 4 * q < K) t = *reinterpret_cast<const float4*>(p + k + 4 * q);   // K % 4 == 0: all in or all out
            v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < PER; ++j) v[j] = (row_ok && k + j < K) ? p[k + j] : 0.0f;
    }
}

// r_m of one row, in every lane of the wave that owns it: get(k) is relu?(x[m,k])
template <class Get>
__device__ __forceinline__ float row_inv_norm(int K, int lane, Get get)
{
    float ss = 0.0f;
    for (int k = lane; k < K; k += 64) {
        const float u = get(k);
        ss += u * u;
    }
    ss = wave_sum(ss);
    return 1.0f / (1e-12f + sqrtf(ss));                                         // model.py:45-46
}

// BatchNorm of column k as one affine map: BN(u)_k = u * mul_k + add_k (g, be: 1 and 0 without the affine parameters)
__device__ __forceinline__ void bn_affine(float mu, float is, float g, float be, float* mul, float* add)
{
    *mul = g * is; *add = be - mu * (g * is);
}

// a[m,k] from x[m,k]: the A operand of an eval block (rm, mu, ad are read only under their flags)
__device__ __forceinline__ float eval_prologue(float v, bool relu, bool has_r, float rm, bool has_bn, float mu, float ad)
{
    if (relu) v = relu_nan(v);
    if (has_r) v = v * rm;
    if (has_bn) v = v * mu + ad;
    return v;
}

// ---- row scales: one wave per row, lanes over columns, then the butterfly
__global__ void __launch_bounds__(kBlock)
mlp_eval_row_kernel(const float* __restrict__ x, long long M, int K, int relu, float* __restrict__ r)
{
    const int lane = threadIdx.x & 63;
    const long long n_waves = (long long)gridDim.x * (kBlock / 64);
    for (long long m = (long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); m < M; m += n_waves) {
        const float* xr = x + m * K;
        const float rm = row_inv_norm(K, lane, [&](int k) { return relu ? relu_nan(xr[k]) : xr[k]; });
        if (lane == 0) r[m] = rm;
    }
}

// ---- the running statistics folded into one affine map per column: BN(u)_k = u * mul_k + add_k
__global__ void __launch_bounds__(kBlock)
mlp_eval_fold_kernel(int K, const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ rmean,
                     const float* __restrict__ rvar, float eps, float* __restrict__ mul, float* __restrict__ add)
{
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= K) return;
    const float mu = rmean[k], is = 1.0f / sqrtf(rvar[k] + eps);
    bn_affine(mu, is, gamma ? gamma[k] : 1.0f, beta ? beta[k] : 0.0f, &mul[k], &add[k]);
}

// ---- host: r[M] of x [M x K]
inline int launch_row_scales(const float* x, long long M, int K, int relu, float* r, hipStream_t st)
{
    const long long grid = cdiv(M, kBlock / 64);
    hipLaunchKernelGGL(mlp_eval_row_kernel, dim3((u32)(grid < kMaxGrid ? grid : kMaxGrid)), dim3(kBlock), 0, st, x, M, K, relu, r);
    return launch_status("mlp_eval_row_kernel");
}

// ---- host: mul[K], then add[K] right behind it
inline int launch_bn_fold(int K, const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                          float* mul, hipStream_t st)
{
    hipLaunchKernelGGL(mlp_eval_fold_kernel, dim3((u32)cdiv(K, kBlock)), dim3(kBlock), 0, st, K, gamma, beta, mean, var, eps, mul,
                       mul + K);
    return launch_status("mlp_eval_fold_kernel");
}

}  // namespace
