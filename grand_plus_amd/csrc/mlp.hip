// mlp.hip -- GRAND+'s MLP on MI355X, one block for all S <= 16 samples of a training step in one set of
// launches.  Reference MLP.forward (model.py:48-66, model_mag.py:57-67): every layer is
//
//     block(x) = Linear( dropout_p( BN( node_norm( relu?(x) ) ) ) )        node_norm(u) = u / (1e-12 + |u|_2)
//
// on x [S x B x F_in] (sample-major, what random_prop*(samples=S) returns), with BatchNorm's batch statistics taken
// per sample over its own B rows (the reference calls the MLP once per sample).  Forward:
//   mlp_row_kernel        one wave per row: r_m = 1 / (1e-12 + |relu?(x_m)|_2)                      (node_norm only)
//   mlp_bn_stats_kernel   16 columns x 16 row groups per workgroup: per sample the mean and biased variance in a fixed
//                         order, the per-column affine map, the running-statistics update in sample order; in eval
//                         mode only the running statistics folded into the affine map                  (BN only)
//   mlp_gemm_kernel       y = a W^T + bias with fp32-input MFMA (16x16x4); a = drop(BN(r * relu?(x))) is computed while
//                         the A tile is staged (the prologue), never a separate pass over HBM
//   mlp_reduce_kernel     the split-K partials summed in split order, then the bias                     (split only)
// Backward: dA = dY W (GEMM), BN's column sums and dn (mlp_bn_backward_kernel), the row norm and ReLU
// (mlp_row_backward_kernel, only when dX is wanted), dW = dY^T a over the saved a (GEMM, split-M partials summed in a
// fixed order), db (mlp_colsum_kernel).  No atomics anywhere: every result is bitwise reproducible.
#include "mlp_eval.hpp"

namespace {

constexpr int kTile = 64;             // GEMM output tile (rows and columns); kBK = 16 deep per step: 4 MFMA k-steps
constexpr int kLdsStride = kTile + 16;
constexpr int kMaxS = 16;
constexpr long long kTargetTiles = 128;   // split the reduction until about this many tiles per sample exist
constexpr long long kMaxSplits = 32;

// Everything the A-operand prologue (and the backward, which applies the same maps) needs.
struct Block {
    const float* x;                 // [M x K], M = S * B
    long long B; int S; int K;
    int relu;
    const float* r;                 // [M] row scales, or NULL (no node_norm)
    const float* mean; const float* invstd; const float* mul; const float* add;   // [S x K] (stride 0 in eval), or NULL (no BN)
    int sstride;                    // K in training, 0 in eval
    int drop; float p, scale; u64 seed; int layer; const unsigned char* keep;    // keep: [S x B x K] or NULL
};

__device__ __forceinline__ float drop_scale(const Block& P, long long s, long long b, int k)
{
    if (!P.drop) return 1.0f;
    const long long e = b * P.K + k;                // the counter hash on the seed of (sample s, layer), or the mask
    if (P.keep) return P.keep[s * P.B * P.K + e] ? P.scale : 0.0f;
    return keep_scale(layer_sample_seed(P.seed, (int)s, P.layer), (u64)e, P.p, P.scale);
}

// n = r * relu?(x): the BatchNorm input
__device__ __forceinline__ float norm_in(const Block& P, float v, long long m)
{
    if (P.relu) v = fmaxf(v, 0.0f);
    if (P.r) v = v * P.r[m];
    return v;
}

__device__ __forceinline__ float prologue(const Block& P, float v, long long m, int k)
{
    v = norm_in(P, v, m);
    const long long s = m / P.B, b = m - s * P.B;
    if (P.mul) v = v * P.mul[s * P.sstride + k] + P.add[s * P.sstride + k];
    if (P.drop) v = v * drop_scale(P, s, b, k);
    return v;
}

// ---- GEMM: C(m, n) = sum_k A(m, k) Bm(k, n), the reduction cut into chunks of kc (a multiple of kBK): chunk z of an
// output element is one MFMA fma chain in k order, and chunks are summed in z order by mlp_reduce_kernel.  How an element
// is computed depends on (K, kc) only, never on which tile or how many rows: the sample-independence contract.
struct Gemm {
    const float* A; long long sam, sak;
    const float* Bm; long long sbk, sbn;
    long long M, N, K, kc;
    float* C; long long ldc;        // nsplit == 1: the result (+ bias); else partial z at C + z * M * ldc
    const float* bias;
    int nsplit;
    float* save_a;                  // forward: the prologue's a [M x K], written by the column-tile-0 workgroups
};

template <bool A_KC, bool B_KC, bool PRO>
__global__ void __launch_bounds__(kBlock)
mlp_gemm_kernel(Gemm g, Block P)
{
    __shared__ float As[kBK][kLdsStride];
    __shared__ float Bs[kBK][kLdsStride];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const long long m0 = (long long)blockIdx.x * kTile, n0 = (long long)blockIdx.y * kTile;
    const long long kbeg = (long long)blockIdx.z * g.kc;
    const long long kend = kbeg + g.kc < g.K ? kbeg + g.kc : g.K;
    const bool save = PRO && g.save_a && blockIdx.y == 0;
    float ra[4], rb[4];
    auto load = [&](long long k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = t + kBlock * i;
            const int kk = A_KC ? (idx & 15) : (idx >> 6), mm = A_KC ? (idx >> 4) : (idx & 63);
            const long long gm = m0 + mm, gk = k0 + kk;
            float v = 0.0f;
            if (gm < g.M && gk < kend) {
                v = g.A[gm * g.sam + gk * g.sak];
                if (PRO) {
                    v = prologue(P, v, gm, (int)gk);
                    if (save) g.save_a[gm * g.K + gk] = v;
                }
            }
            ra[i] = v;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = t + kBlock * i;
            const int kk = B_KC ? (idx & 15) : (idx >> 6), nn = B_KC ? (idx >> 4) : (idx & 63);
            const long long gn = n0 + nn, gk = k0 + kk;
            rb[i] = (gn < g.N && gk < kend) ? g.Bm[gk * g.sbk + gn * g.sbn] : 0.0f;
        }
    };
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (kbeg < kend) load(kbeg);
    for (long long k0 = kbeg; k0 < kend; k0 += kBK) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = t + kBlock * i;
            As[A_KC ? (idx & 15) : (idx >> 6)][A_KC ? (idx >> 4) : (idx & 63)] = ra[i];
            Bs[B_KC ? (idx & 15) : (idx >> 6)][B_KC ? (idx >> 4) : (idx & 63)] = rb[i];
        }
        __syncthreads();
        if (k0 + kBK < kend) load(k0 + kBK);                 // next tile in flight while this one is multiplied
#pragma unroll
        for (int ks = 0; ks < kBK / 4; ++ks) {
            const int kr = ks * 4 + (lane >> 4);             // 16x16x4: lane holds A[l&15][l>>4], B[l>>4][l&15]
            float a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = As[kr][wm * 32 + i * 16 + (lane & 15)];
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = Bs[kr][wn * 32 + j * 16 + (lane & 15)];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }
    float* C = g.C + (g.nsplit > 1 ? (long long)blockIdx.z * g.M * g.ldc : 0);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const long long col = n0 + wn * 32 + j * 16 + (lane & 15);   // C/D: col = lane & 15, row = 4 (lane >> 4) + reg
            if (col >= g.N) continue;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const long long row = m0 + wm * 32 + i * 16 + (lane >> 4) * 4 + q;
                if (row >= g.M) continue;
                float v = acc[i][j][q];
                if (g.nsplit == 1 && g.bias) v = v + g.bias[col];
                C[row * g.ldc + col] = v;
            }
        }
}

// out[i] = ((part_0[i] + part_1[i]) + ...) (+ bias[i % N]), out and the partials dense [M x N]
__global__ void __launch_bounds__(kBlock)
mlp_reduce_kernel(const float* __restrict__ part, int nsplit, long long total, long long N, const float* __restrict__ bias,
                  float* __restrict__ out)
{
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kBlock) {
        float v = part[i];
        for (int z = 1; z < nsplit; ++z) v = v + part[(long long)z * total + i];
        if (bias) v = v + bias[i % N];
        out[i] = v;
    }
}

// ---- row scales: one wave per row, lanes over columns, then a butterfly (fixed order)
__global__ void __launch_bounds__(kBlock)
mlp_row_kernel(Block P, long long M, float* __restrict__ r)
{
    const int lane = threadIdx.x & 63;
    const long long n_waves = (long long)gridDim.x * (kBlock / 64);
    for (long long m = (long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); m < M; m += n_waves) {
        const float* xr = P.x + m * P.K;
        const float rm = row_inv_norm(P.K, lane, [&](int k) { return P.relu ? fmaxf(xr[k], 0.0f) : xr[k]; });
        if (lane == 0) r[m] = rm;
    }
}

// 16 columns per workgroup (tx), 16 row groups (ty): a column sum over rows b = ty, ty + 16, ... and then a fixed tree.
__device__ __forceinline__ float col_reduce(float v, float (*red)[17], int tx, int ty)
{
    red[ty][tx] = v;
    __syncthreads();
    for (int h = 8; h > 0; h >>= 1) {
        if (ty < h) red[ty][tx] = red[ty][tx] + red[ty + h][tx];
        __syncthreads();
    }
    const float out = red[0][tx];
    __syncthreads();
    return out;
}

struct BnArgs {
    const float* gamma; const float* beta;
    float* rmean; float* rvar; long long* nbt;
    float eps, momentum;
    int training;
    float* mean; float* invstd; float* mul; float* add;
};

__global__ void __launch_bounds__(kBlock)
mlp_bn_stats_kernel(Block P, BnArgs a)
{
    __shared__ float red[16][17];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int k = blockIdx.x * 16 + tx;
    const bool col = k < P.K;
    if (!a.training) {                               // eval: fold the running statistics into one affine map
        if (col && ty == 0) {
            const float mu = a.rmean[k], is = 1.0f / sqrtf(a.rvar[k] + a.eps);
            const float g = a.gamma ? a.gamma[k] : 1.0f, be = a.beta ? a.beta[k] : 0.0f;
            a.mean[k] = mu; a.invstd[k] = is;
            bn_affine(mu, is, g, be, &a.mul[k], &a.add[k]);
        }
        return;
    }
    const float inv_b = 1.0f / (float)P.B;
    for (int s = 0; s < P.S; ++s) {
        const long long base = (long long)s * P.B;
        float sum = 0.0f;
        if (col)
            for (long long b = ty; b < P.B; b += 16) sum += norm_in(P, P.x[(base + b) * P.K + k], base + b);
        const float mu = col_reduce(sum, red, tx, ty) * inv_b;
        float sq = 0.0f;
        if (col)
            for (long long b = ty; b < P.B; b += 16) {
                const float d = norm_in(P, P.x[(base + b) * P.K + k], base + b) - mu;
                sq += d * d;
            }
        const float var = col_reduce(sq, red, tx, ty) * inv_b;                  // biased: normalisation uses it
        if (col && ty == 0) {
            const float is = 1.0f / sqrtf(var + a.eps);
            const float g = a.gamma ? a.gamma[k] : 1.0f, be = a.beta ? a.beta[k] : 0.0f;
            const long long o = (long long)s * P.K + k;
            a.mean[o] = mu; a.invstd[o] = is;
            bn_affine(mu, is, g, be, &a.mul[o], &a.add[o]);
            if (a.rmean) {                           // once per sample, in sample order, as S calls of bn(x)
                const float m = a.momentum;
                a.rmean[k] = (1.0f - m) * a.rmean[k] + m * mu;
                a.rvar[k] = (1.0f - m) * a.rvar[k] + m * (var * ((float)P.B / (float)(P.B - 1)));
            }
        }
    }
    if (a.nbt && blockIdx.x == 0 && threadIdx.x == 0) *a.nbt = *a.nbt + P.S;
}

// BatchNorm backward per column: dy = dA * keep, per sample the sums of dy and dy * xhat (fixed order), dgamma / dbeta
// summed over samples in order; with write_dn dA is overwritten by dn, the gradient at BatchNorm's input.
__global__ void __launch_bounds__(kBlock)
mlp_bn_backward_kernel(Block P, const float* __restrict__ gamma, int training, float* dA, int write_dn,
                       float* __restrict__ dgamma, float* __restrict__ dbeta)
{
    __shared__ float red[16][17];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int k = blockIdx.x * 16 + tx;
    const bool col = k < P.K;
    const float g = (col && gamma) ? gamma[k] : 1.0f;
    const float inv_b = 1.0f / (float)P.B;
    float gacc = 0.0f, bacc = 0.0f;
    for (int s = 0; s < P.S; ++s) {
        const long long base = (long long)s * P.B;
        const float mu = col ? P.mean[s * P.sstride + k] : 0.0f, is = col ? P.invstd[s * P.sstride + k] : 0.0f;
        float sdy = 0.0f, sdx = 0.0f;
        if (col)
            for (long long b = ty; b < P.B; b += 16) {
                const long long m = base + b;
                const float dy = dA[m * P.K + k] * drop_scale(P, s, b, k);
                const float xh = (norm_in(P, P.x[m * P.K + k], m) - mu) * is;
                sdy += dy;
                sdx += dy * xh;
            }
        sdy = col_reduce(sdy, red, tx, ty);
        sdx = col_reduce(sdx, red, tx, ty);
        gacc = gacc + sdx;
        bacc = bacc + sdy;
        if (write_dn && col) {
            const float c = g * is, mdy = sdy * inv_b, mdx = sdx * inv_b;
            for (long long b = ty; b < P.B; b += 16) {
                const long long m = base + b;
                const float dy = dA[m * P.K + k] * drop_scale(P, s, b, k);
                float dn;
                if (training) {
                    const float xh = (norm_in(P, P.x[m * P.K + k], m) - mu) * is;
                    dn = ((dy - mdy) - xh * mdx) * c;
                } else {
                    dn = dy * c;
                }
                dA[m * P.K + k] = dn;
            }
        }
    }
    if (col && ty == 0) {
        if (dgamma) dgamma[k] = gacc;
        if (dbeta) dbeta[k] = bacc;
    }
}

// dX per row: g = dn (after BN) or dA * keep; node_norm's Jacobian du = r g - u r^2 / |u| <g, u>; then ReLU's mask.
__global__ void __launch_bounds__(kBlock)
mlp_row_backward_kernel(Block P, long long M, int bn, const float* __restrict__ g, float* __restrict__ dx)
{
    const int lane = threadIdx.x & 63;
    const long long n_waves = (long long)gridDim.x * (kBlock / 64);
    for (long long m = (long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); m < M; m += n_waves) {
        const long long s = m / P.B, b = m - s * P.B;
        const float* xr = P.x + m * P.K;
        const float* gr = g + m * P.K;
        float c = 0.0f, rr = 0.0f;
        if (P.r) {
            float ss = 0.0f, dot = 0.0f;
            for (int k = lane; k < P.K; k += 64) {
                const float u = P.relu ? fmaxf(xr[k], 0.0f) : xr[k];
                const float gv = bn ? gr[k] : gr[k] * drop_scale(P, s, b, k);
                ss += u * u;
                dot += gv * u;
            }
            ss = wave_sum(ss);
            dot = wave_sum(dot);
            const float L = sqrtf(ss);
            rr = P.r[m];
            c = L > 0.0f ? rr * rr / L * dot : 0.0f;
        }
        for (int k = lane; k < P.K; k += 64) {
            const float xv = xr[k];
            float gv = bn ? gr[k] : gr[k] * drop_scale(P, s, b, k);
            if (P.r) gv = rr * gv - (P.relu ? fmaxf(xv, 0.0f) : xv) * c;
            if (P.relu && !(xv > 0.0f)) gv = 0.0f;
            dx[m * P.K + k] = gv;
        }
    }
}

// db[n] = sum_m dY[m, n] in a fixed order
__global__ void __launch_bounds__(kBlock)
mlp_colsum_kernel(const float* __restrict__ dy, long long M, int N, float* __restrict__ out)
{
    __shared__ float red[16][17];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int n = blockIdx.x * 16 + tx;
    float sum = 0.0f;
    if (n < N)
        for (long long m = ty; m < M; m += 16) sum += dy[m * N + n];
    sum = col_reduce(sum, red, tx, ty);
    if (n < N && ty == 0) out[n] = sum;
}

// ---- host side
// chunk of the reduction dimension: enough splits that the (row tiles x column tiles) of one sample reach kTargetTiles,
// at least 64 deep each, at most kMaxSplits
long long k_chunk(long long tiles, long long K)
{
    long long want = tiles >= kTargetTiles ? 1 : kTargetTiles / tiles;
    const long long most = cdiv(K, 64);
    if (want > most) want = most;
    if (want > kMaxSplits) want = kMaxSplits;
    if (want < 1) want = 1;
    return cdiv(cdiv(K, kBK), want) * kBK;
}

int grid1(long long n, long long per)
{
    const long long g = cdiv(n, per);
    return (int)(g < 65535 ? (g > 0 ? g : 1) : 65535);
}

template <bool A_KC, bool B_KC, bool PRO>
int run_gemm(Gemm g, const Block& P, void* ws, hipStream_t st, const char* name)
{
    float* out = g.C;
    const long long kc = g.kc;
    g.nsplit = (int)cdiv(g.K, kc);
    if (g.nsplit > 1) g.C = static_cast<float*>(ws);
    const long long gx = cdiv(g.M, kTile), gy = cdiv(g.N, kTile);
    hipLaunchKernelGGL((mlp_gemm_kernel<A_KC, B_KC, PRO>), dim3((u32)gx, (u32)gy, (u32)g.nsplit), dim3(kBlock), 0, st, g, P);
    if (const int rc = launch_status(name)) return rc;
    if (g.nsplit > 1) {
        const long long total = g.M * g.N;
        hipLaunchKernelGGL(mlp_reduce_kernel, dim3(grid1(total, kBlock)), dim3(kBlock), 0, st, (const float*)g.C, g.nsplit, total,
                           g.N, g.bias, out);
        return launch_status("mlp_reduce_kernel");
    }
    return GP_OK;
}

int check_common(const char* where, const float* d_x, int32_t S, int64_t B, int32_t f_in, int32_t f_out, const float* d_w,
                 int flags, float dropout)
{
    if (S < 1 || S > kMaxS || B < 1 || f_in < 1 || f_out < 1 || (flags & ~0xF) || !(dropout >= 0.0f && dropout <= 1.0f))
        return fail(GP_ERR_INVALID_ARG, where, "n_samples outside [1, 16], n_rows < 1, f_in < 1, f_out < 1, unknown flags or "
                                               "dropout outside [0, 1]");
    if ((long long)S * B > (1ll << 40) || (long long)f_in * f_out > (1ll << 40) || f_out > (1 << 22))
        return fail(GP_ERR_INVALID_ARG, where, "sizes out of range");
    if ((flags & GP_MLP_BN) && (flags & GP_MLP_TRAINING) && B < 2)
        return fail(GP_ERR_INVALID_ARG, where, "BatchNorm in training needs more than 1 row per sample");
    if (!d_x || !d_w) return fail(GP_ERR_NULL, where, "a device pointer is NULL");
    return GP_OK;
}

Block make_block(const float* d_x, int32_t S, int64_t B, int32_t f_in, int flags, float dropout, uint64_t seed, int32_t layer,
                 const uint8_t* d_keep, const float* saved)
{
    Block P = {};
    P.x = d_x; P.B = B; P.S = S; P.K = f_in;
    P.relu = (flags & GP_MLP_RELU) != 0;
    const long long M = (long long)S * B;
    const bool training = (flags & GP_MLP_TRAINING) != 0;
    P.r = (flags & GP_MLP_NORM) ? saved : nullptr;
    if (flags & GP_MLP_BN) {
        const float* st = saved + M;
        const long long n = (long long)S * f_in;
        P.mean = st; P.invstd = st + n; P.mul = st + 2 * n; P.add = st + 3 * n;
        P.sstride = training ? f_in : 0;
    }
    P.drop = training && dropout > 0.0f;
    P.p = dropout;
    P.scale = dropout < 1.0f ? 1.0f / (1.0f - dropout) : 0.0f;           // p = 1: zeros, as torch
    P.seed = seed; P.layer = layer; P.keep = d_keep;
    return P;
}

}  // namespace

extern "C" {

int gp_mlp_block_forward(int device, const float* d_x, int32_t n_samples, int64_t n_rows, int32_t f_in, int32_t f_out,
                         const float* d_weight, const float* d_bias, int flags,
                         const float* d_bn_weight, const float* d_bn_bias, float* d_running_mean, float* d_running_var,
                         int64_t* d_num_batches_tracked, float bn_eps, float bn_momentum,
                         float dropout, uint64_t seed, int32_t layer, const uint8_t* d_keep,
                         float* d_out, float* d_saved, float* d_saved_a, void* d_workspace, void* stream)
{
    const char* where = "gp_mlp_block_forward";
    if (const int rc = check_common(where, d_x, n_samples, n_rows, f_in, f_out, d_weight, flags, dropout)) return rc;
    const bool bn = (flags & GP_MLP_BN) != 0, training = (flags & GP_MLP_TRAINING) != 0;
    if (bn && (!(bn_eps > 0.0f) || !(bn_momentum >= 0.0f && bn_momentum <= 1.0f)))
        return fail(GP_ERR_INVALID_ARG, where, "bn_eps <= 0 or bn_momentum outside [0, 1]");
    if (!d_out || !d_workspace || ((flags & (GP_MLP_NORM | GP_MLP_BN)) && !d_saved) || (bn && !training && (!d_running_mean || !d_running_var)) ||
        (bn && (!d_running_mean) != (!d_running_var)))
        return fail(GP_ERR_NULL, where, "a device pointer is NULL");
    if (const int rc = set_device(device, where)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const long long M = (long long)n_samples * n_rows;
    const Block P = make_block(d_x, n_samples, n_rows, f_in, flags, dropout, seed, layer, d_keep, d_saved);
    if (flags & GP_MLP_NORM) {
        hipLaunchKernelGGL(mlp_row_kernel, dim3(grid1(M, kBlock / 64)), dim3(kBlock), 0, st, P, M, d_saved);
        if (const int rc = launch_status("mlp_row_kernel")) return rc;
    }
    if (bn) {
        float* s0 = d_saved + M;
        const long long n = (long long)n_samples * f_in;
        const BnArgs a = {d_bn_weight, d_bn_bias, d_running_mean, d_running_var, (long long*)d_num_batches_tracked, bn_eps,
                          bn_momentum, training, s0, s0 + n, s0 + 2 * n, s0 + 3 * n};
        hipLaunchKernelGGL(mlp_bn_stats_kernel, dim3((u32)cdiv(f_in, 16)), dim3(kBlock), 0, st, P, a);
        if (const int rc = launch_status("mlp_bn_stats_kernel")) return rc;
    }
    Gemm g = {};
    g.A = d_x; g.sam = f_in; g.sak = 1;
    g.Bm = d_weight; g.sbk = 1; g.sbn = f_in;
    g.M = M; g.N = f_out; g.K = f_in;
    g.kc = k_chunk(cdiv(n_rows, kTile) * cdiv(f_out, kTile), f_in);     // from one sample's shape: independent of S
    g.C = d_out; g.ldc = f_out; g.bias = d_bias; g.save_a = d_saved_a;
    return run_gemm<true, true, true>(g, P, d_workspace, st, "mlp_gemm_kernel<fwd>");
}

int gp_mlp_block_backward(int device, const float* d_x, int32_t n_samples, int64_t n_rows, int32_t f_in, int32_t f_out,
                          const float* d_weight, int flags, const float* d_bn_weight,
                          float dropout, uint64_t seed, int32_t layer, const uint8_t* d_keep,
                          const float* d_saved, const float* d_saved_a, const float* d_grad_out,
                          float* d_grad_x, float* d_grad_weight, float* d_grad_bias, float* d_grad_bn_weight, float* d_grad_bn_bias,
                          void* d_workspace, void* stream)
{
    const char* where = "gp_mlp_block_backward";
    if (const int rc = check_common(where, d_x, n_samples, n_rows, f_in, f_out, d_weight, flags, dropout)) return rc;
    const bool bn = (flags & GP_MLP_BN) != 0, training = (flags & GP_MLP_TRAINING) != 0;
    const bool want_bn = bn && (d_grad_bn_weight || d_grad_bn_bias);
    const bool need_da = d_grad_x || want_bn;
    if (!d_grad_out || !d_workspace || ((flags & (GP_MLP_NORM | GP_MLP_BN)) && !d_saved) || (d_grad_weight && !d_saved_a))
        return fail(GP_ERR_NULL, where, "a device pointer is NULL");
    if (const int rc = set_device(device, where)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const long long M = (long long)n_samples * n_rows;
    const Block P = make_block(d_x, n_samples, n_rows, f_in, flags, dropout, seed, layer, d_keep, d_saved);
    float* dA = static_cast<float*>(d_workspace);                    // [M x f_in], then the split partials
    float* part = dA + M * f_in;
    if (need_da) {
        Gemm g = {};
        g.A = d_grad_out; g.sam = f_out; g.sak = 1;
        g.Bm = d_weight; g.sbk = f_in; g.sbn = 1;
        g.M = M; g.N = f_in; g.K = f_out;
        g.kc = k_chunk(cdiv(M, kTile) * cdiv(f_in, kTile), f_out);
        g.C = dA; g.ldc = f_in;
        if (const int rc = run_gemm<true, false, false>(g, P, part, st, "mlp_gemm_kernel<dA>")) return rc;
        if (bn) {
            hipLaunchKernelGGL(mlp_bn_backward_kernel, dim3((u32)cdiv(f_in, 16)), dim3(kBlock), 0, st, P, d_bn_weight,
                               (int)training, dA, d_grad_x ? 1 : 0, d_grad_bn_weight, d_grad_bn_bias);
            if (const int rc = launch_status("mlp_bn_backward_kernel")) return rc;
        }
        if (d_grad_x) {
            hipLaunchKernelGGL(mlp_row_backward_kernel, dim3(grid1(M, kBlock / 64)), dim3(kBlock), 0, st, P, M, (int)bn,
                               (const float*)dA, d_grad_x);
            if (const int rc = launch_status("mlp_row_backward_kernel")) return rc;
        }
    }
    if (d_grad_weight) {                             // dW[n, k] = sum_m dY[m, n] a[m, k], split over m
        Gemm g = {};
        g.A = d_grad_out; g.sam = 1; g.sak = f_out;
        g.Bm = d_saved_a; g.sbk = f_in; g.sbn = 1;
        g.M = f_out; g.N = f_in; g.K = M;
        g.kc = k_chunk(cdiv(f_out, kTile) * cdiv(f_in, kTile), M);
        g.C = d_grad_weight; g.ldc = f_in;
        if (const int rc = run_gemm<false, false, false>(g, P, part, st, "mlp_gemm_kernel<dW>")) return rc;
    }
    if (d_grad_bias) {
        hipLaunchKernelGGL(mlp_colsum_kernel, dim3((u32)cdiv(f_out, 16)), dim3(kBlock), 0, st, d_grad_out, M, f_out, d_grad_bias);
        if (const int rc = launch_status("mlp_colsum_kernel")) return rc;
    }
    return GP_OK;
}

}  // extern "C"
