// gp_common.hpp -- what the translation units outside GFPush share (augment.hip, evaluate.hip, mag_prop.hip,
// objective.hip, optim.hip, propagate.hip, scatter_det.hip, and through mlp_eval.hpp mlp.hip, mlp_infer.hip and
// mlp_chain.hip): the dropout counter hash and the seed derivations that grandplus.h fixes bit for bit, the wave
// and workgroup reductions, the float vector map, and the host helpers every entry point uses (error record, device selection,
// launch status, feature-column launch geometry).  Everything has internal linkage: no symbol leaves a translation unit.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "grandplus.h"

namespace {

typedef unsigned long long u64;
typedef unsigned int u32;

// ---- device: seeds and the dropout hash (the only definition of these formulas on the device)
__device__ __forceinline__ u64 fmix64(u64 x)                 // splitmix64's finaliser
{
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__device__ __forceinline__ u64 mix64(u64 x) { return fmix64(x + 0x9E3779B97F4A7C15ull); }

// gp_sample_seed of grandplus.h: the seed of sample s of an S-sample call, seed itself for s = 0
__device__ __forceinline__ u64 sample_seed(u64 seed, int s)
{
    return s == 0 ? seed : mix64(seed ^ ((u64)s * 0xD6E8FEB86659FD93ull));
}

// GP_MLP_LAYER_SEED(gp_sample_seed(seed, s), layer): the MLP's dropout seed of (sample s, layer)
__device__ __forceinline__ u64 layer_sample_seed(u64 seed, int s, int layer)
{
    return mix64(sample_seed(seed, s) ^ ((u64)(layer + 1) * 0xA0761D6478BD642Full));
}

// counter-based RNG: one 24-bit uniform per (seed, entry); keep with probability 1-p
__device__ __forceinline__ float keep_scale(u64 seed, u64 entry, float p, float scale)
{
    const u64 x = fmix64(seed + entry * 0x9E3779B97F4A7C15ull);
    const float u = (float)(u32)(x >> 40) * (1.0f / 16777216.0f);
    return u >= p ? scale : 0.0f;
}

// ---- device: wave butterflies (every lane ends with the result; a fixed order, so bitwise reproducible)
__device__ __forceinline__ float wave_sum(float v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ float wave_max(float v)
{
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// The sum of v over a workgroup of NW waves, in every thread, through lds[NW] (T: double, long long).  A fixed tree: the
// xor butterfly inside a wave (both partners add the same two values), then the waves in order.
template <int NW, class T>
__device__ __forceinline__ T block_sum(T v, T* lds)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    T s = lds[0];
    for (int w = 1; w < NW; ++w) s += lds[w];
    return s;
}

// ---- device: VEC floats per lane per access
template <int VEC> struct VecT;
template <> struct VecT<4> { typedef float4 type; };
template <> struct VecT<2> { typedef float2 type; };
template <> struct VecT<1> { typedef float type; };

// ---- host
inline int fail(int status, const char* where, const char* detail)      // record the error, return its code
{
    gp_internal_set_error(status, where, detail);
    return status;
}

inline int set_device(int device, const char* where)
{
    const hipError_t e = hipSetDevice(device);
    return e == hipSuccess ? GP_OK : fail(GP_ERR_NO_DEVICE, where, hipGetErrorString(e));
}

inline int launch_status(const char* where)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GP_OK : fail(GP_ERR_HIP, where, hipGetErrorString(e));
}

// Launch geometry over F feature columns: the widest vector that divides F, and how many slabs of lanes * vec
// columns cover F (lanes: the threads that span the columns, a workgroup or a wave).
inline int vec_width(int F) { return (F & 3) == 0 ? 4 : (F & 1) == 0 ? 2 : 1; }
inline int feature_slabs(int F, int vec, int lanes) { return (F + lanes * vec - 1) / (lanes * vec); }

// workgroups of `waves` waves for a kernel whose waves take rows grid-stride: at least one, at most 65 535
inline int row_grid(long long n, int waves)
{
    const long long g = (n + waves - 1) / waves;
    return (int)(g < 65535 ? (g > 0 ? g : 1) : 65535);
}

// log2 of the smallest lane group G with G * vec >= F, at most a wave: a wave then handles 64 / G rows at once
inline int lane_group_log2(int F, int vec)
{
    int log2g = 0;
    while (log2g < 6 && (1 << log2g) * vec < F) ++log2g;
    return log2g;
}

}  // namespace
