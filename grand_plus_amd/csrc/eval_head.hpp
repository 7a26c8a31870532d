// eval_head.hpp -- the row arithmetic of the evaluation head, stated once for eval_head_kernel (evaluate.hip)
// and eval_tail_kernel (eval_tail.hip): one wave per evaluated row gives nll, pred and a flag.  HIP only;
// everything has internal linkage, as gp_common.hpp's.
#pragma once

#include "gp_common.hpp"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxC = 4096;

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

// The rows of a grid of kBlock-thread workgroups, one wave per row, grid-stride: nll, pred and flag at a.offset + i.  A macro,
// expanded in the body of each of the two kernels with its own parameter names: the kernels then compile to what the text
// in place compiles to (an inlined function did not: evaluate.hip's device code has to stay what it was).
#define GP_EVAL_HEAD_ROWS(a, nll, pred, flag) \
{ \
    const int lane = threadIdx.x & 63; \
    const long long n_waves = (long long)gridDim.x * kWaves; \
    for (long long i = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6); i < a.n; i += n_waves) {   /* wave-uniform */ \
        const long long r = a.row_idx ? a.row_idx[i] : i; \
        const long long l = a.label_idx ? a.label_idx[i] : i; \
        float loss = 0.0f; int arg = -1; int fl = kBad; \
        if (r >= 0 && r < a.n_z) {                  /* an index outside its array is never used as an address */ \
            const float* __restrict__ zr = a.z + (size_t)r * a.C; \
            /* the first 64 classes stay in a register: one read of the row for C <= 64 */ \
            const float z0 = lane < a.C ? zr[lane] : -INFINITY; \
            float best = z0; arg = lane < a.C ? lane : 0x7FFFFFFF; \
            for (int c = lane + 64; c < a.C; c += 64) { \
                const float v = zr[c]; \
                if (better(v, c, best, arg)) { best = v; arg = c; } \
            } \
            for (int o = 32; o > 0; o >>= 1) { \
                const float ob = __shfl_xor(best, o); const int oa = __shfl_xor(arg, o); \
                if (better(ob, oa, best, arg)) { best = ob; arg = oa; } \
            } \
            if (l >= 0 && l < a.n_labels) { \
                const long long y = a.labels[l]; \
                if (y == a.ignore) fl = kIgnored; \
                else if (y >= 0 && y < a.C) { \
                    /* (z - max) - log sum exp(z - max), the objective's order; a NaN in the row is the max: NaN, as torch */ \
                    float e = lane < a.C ? expf(z0 - best) : 0.0f; \
                    for (int c = lane + 64; c < a.C; c += 64) e += expf(zr[c] - best); \
                    const float ls = logf(wave_sum(e)); \
                    loss = -((zr[y] - best) - ls); \
                    fl = arg == y ? kCorrect : kWrong; \
                } \
            } \
        } \
        if (lane == 0) { nll[a.offset + i] = loss; pred[a.offset + i] = arg; flag[a.offset + i] = (unsigned char)fl; } \
    } \
}

}  // namespace
