// mlp_infer.hip -- the eval-only MLP block over any number of rows, on a GEMM sized for M >> N.  One layer
// per call (gp_mlp_infer_block, grandplus_infer.h):
//
//     y[M x N] = a W^T + b,      a = BN_running( node_norm( relu?(x) ) ),      node_norm(u) = u / (1e-12 + |u|_2)
//
//   mlp_eval_row_kernel    one wave per row: r_m = 1 / (1e-12 + |relu?(x_m)|_2)                        (GP_MLP_NORM only)
//   mlp_eval_fold_kernel   the running statistics folded into one affine map per column: mul_k, add_k    (GP_MLP_BN only)
//   mlp_infer_gemm_kernel  fp32-input MFMA; a = (relu?(x) * r_m) * mul_k + add_k is computed while the A tile is staged
//
// The arithmetic contract (one fma chain per output in ascending k, the order of the row sums, the fold, the
// NaN-keeping relu) is mlp_eval.hpp's, which also defines the first two kernels; mlp.hip's eval mode calls the same
// row sum and fold, so a layer equals gp_mlp_block_forward bit for bit wherever that takes one k-chain.  Every
// instantiation here keeps the contract, whatever the tile, M or N.  No sample dimension, dropout or split-K.
//
// The GEMM: 256 threads, k-depth 16 per stage, two LDS stages (the next A/W tile is loaded from global memory while
// the current one is multiplied; one barrier per k-step).
//   wide    (N > 64)   128 x 128 tile, waves 2 x 2, each 64 x 64 = 2 x 2 v_mfma_f32_32x32x2_f32
//   narrow  (N <= 64)  128 x 64 tile,  waves 4 x 1, each 32 x 64 = 2 x ceil(N / 16) v_mfma_f32_16x16x4_f32
// LDS image: one row of 16 k per tile row, 20 floats apart (the 4-float pad makes the 16-byte slot of row r 5 r mod 16:
// ds_read_b128 is conflict-free for the wide tile, at most 2-way for the narrow one).  A lane of 32x32x2 holds
// k = 2 s + (lane >> 5) of step s, a lane of 16x16x4 k = 4 s + (lane >> 4): the k of a row are permuted when they are
// WRITTEN (kperm) so that one ds_read_b128 hands a lane its k of four consecutive steps, and the chain stays in k order.
#include "mlp_eval.hpp"

namespace {

constexpr int kBM = 128;              // rows of an output tile, both instantiations

struct Infer {
    const float* x; long long M; int K; int N;
    const float* w; const float* bias;
    int relu;
    const float* r;                   // [M] row scales, or NULL (no node_norm)
    const float* mul; const float* add;   // [K] the folded BatchNorm, or NULL
    float* y;
    int nct;                          // column tiles
};

// where k (0 ... 15) of a tile row is stored: the permutation of this instantiation's MFMA operand
template <bool WIDE> __device__ __forceinline__ int kperm(int k) { return WIDE ? kperm32(k) : kperm16(k); }

template <bool WIDE, bool VEC>
__global__ void __launch_bounds__(kBlock, 2)
mlp_infer_gemm_kernel(Infer g)
{
    constexpr int BN = WIDE ? 128 : 64;
    constexpr int PA = kBM * kBK / kBlock, PB = BN * kBK / kBlock;     // floats per thread per stage: 8, and 8 or 4
    __shared__ __attribute__((aligned(16))) float lds[2][(kBM + BN) * kStride];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long bid = blockIdx.x;
    const long long m0 = (bid / g.nct) * kBM;
    const int n0 = (int)(bid % g.nct) * BN;

    // staging: this thread's row of the A tile and of the W tile, and its first k inside a stage
    const int ar = t / (kBK / PA), ak = (t % (kBK / PA)) * PA;
    const int br = t / (kBK / PB), bk = (t % (kBK / PB)) * PB;
    const long long am = m0 + ar;
    const bool a_ok = am < g.M, b_ok = n0 + br < g.N;
    const float* ap = g.x + (a_ok ? am : 0) * g.K;
    const float* bp = g.w + (long long)(b_ok ? n0 + br : 0) * g.K;
    const float rm = (g.r && a_ok) ? g.r[am] : 1.0f;
    float xa[PA], wb[PB], mu[PA], ad[PA];
    auto load = [&](int k0) {
        load_row<PA, VEC>(ap, a_ok, k0 + ak, g.K, xa);
        load_row<PB, VEC>(bp, b_ok, k0 + bk, g.K, wb);
        if (g.mul) {
#pragma unroll
            for (int j = 0; j < PA; ++j) {
                const bool ok = k0 + ak + j < g.K;
                mu[j] = ok ? g.mul[k0 + ak + j] : 0.0f;
                ad[j] = ok ? g.add[k0 + ak + j] : 0.0f;
            }
        }
    };
    auto stage = [&](int k0, float* buf) {           // the prologue, then the permuted LDS rows
        float* arow = buf + ar * kStride;
        float* brow = buf + (kBM + br) * kStride;
#pragma unroll
        for (int j = 0; j < PA; ++j) {
            const bool ok = a_ok && k0 + ak + j < g.K;
            const float v = ok ? eval_prologue(xa[j], g.relu, g.r, rm, g.mul, mu[j], ad[j]) : 0.0f;
            arow[kperm<WIDE>(ak + j)] = v;
        }
#pragma unroll
        for (int j = 0; j < PB; ++j) brow[kperm<WIDE>(bk + j)] = wb[j];
    };

    // this wave's fragments
    constexpr int FI = 2, FJ = WIDE ? 2 : 4, FR = WIDE ? 32 : 16, STEPS = WIDE ? 8 : 4;   // fragment rows; MFMA steps per stage
    const int fl = lane & (FR - 1), fh = lane / FR;                   // row / column inside a fragment; which k of a step
    const int wr = WIDE ? (wave & 1) * 64 : wave * 32, wc = WIDE ? (wave >> 1) * 64 : 0;
    const int nfrag = WIDE ? FJ : (g.N - n0 + 15) / 16;               // narrow: column fragments that hold a column
    f32x16 acc32[2][2];
    f32x4 acc16[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc32[i][j][q] = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc16[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }

    const int nst = (g.K + kBK - 1) / kBK;
    load(0);
    stage(0, lds[0]);
    __syncthreads();
    for (int s = 0; s < nst; ++s) {
        const float* buf = lds[s & 1];
        if (s + 1 < nst) load((s + 1) * kBK);                        // in flight while this stage is multiplied
        float a[FI][STEPS], b[FJ][STEPS];
#pragma unroll
        for (int i = 0; i < FI; ++i)
#pragma unroll
            for (int q = 0; q < STEPS / 4; ++q) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(buf + (wr + i * FR + fl) * kStride + fh * STEPS + 4 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e) a[i][4 * q + e] = v[e];
            }
#pragma unroll
        for (int j = 0; j < FJ; ++j)
#pragma unroll
            for (int q = 0; q < STEPS / 4; ++q) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(buf + (kBM + wc + j * FR + fl) * kStride + fh * STEPS + 4 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e) b[j][4 * q + e] = v[e];
            }
#pragma unroll
        for (int ks = 0; ks < STEPS; ++ks)
#pragma unroll
            for (int i = 0; i < FI; ++i)
#pragma unroll
                for (int j = 0; j < FJ; ++j) {
                    if (WIDE) acc32[i][j & 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][ks], b[j][ks], acc32[i][j & 1], 0, 0, 0);
                    else if (j < nfrag) acc16[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][ks], b[j][ks], acc16[i][j], 0, 0, 0);
                }
        if (s + 1 < nst) stage((s + 1) * kBK, lds[(s + 1) & 1]);     // last read before the barrier that ended step s - 1
        __syncthreads();
    }

    // C/D: 32x32: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5); 16x16: col = lane & 15, row = 4 (lane >> 4) + reg
#pragma unroll
    for (int i = 0; i < FI; ++i)
#pragma unroll
        for (int j = 0; j < FJ; ++j) {
            const int col = n0 + wc + j * FR + fl;
            if (col >= g.N) continue;
            const float bv = g.bias ? g.bias[col] : 0.0f;
#pragma unroll
            for (int q = 0; q < (WIDE ? 16 : 4); ++q) {
                const long long row = m0 + wr + i * FR + (WIDE ? (q & 3) + 8 * (q >> 2) + 4 * fh : 4 * fh + q);
                if (row >= g.M) continue;
                float v = WIDE ? acc32[i][j & 1][q] : acc16[i][j][q];
                if (g.bias) v = v + bv;
                g.y[row * g.N + col] = v;
            }
        }
}

// ---- host side
template <bool WIDE>
int run_gemm(Infer g, hipStream_t st)
{
    constexpr int BN = WIDE ? 128 : 64;
    g.nct = (int)cdiv(g.N, BN);
    // float4 loads need 16-byte row starts in both operands: an aligned base and K a multiple of 4
    const bool vec = (g.K & 3) == 0 && (((uintptr_t)g.x | (uintptr_t)g.w) & 15) == 0;
    const long long tiles_per_launch = kMaxGrid / g.nct > 0 ? kMaxGrid / g.nct : 1;
    const long long row_tiles = cdiv(g.M, kBM);
    const long long M = g.M;
    for (long long t0 = 0; t0 < row_tiles; t0 += tiles_per_launch) {       // one launch unless M is beyond 2^29 rows
        const long long nt = row_tiles - t0 < tiles_per_launch ? row_tiles - t0 : tiles_per_launch;
        Infer c = g;
        const long long first = t0 * kBM;
        c.x = g.x + first * g.K; c.y = g.y + first * g.N; c.r = g.r ? g.r + first : nullptr;
        c.M = M - first < nt * kBM ? M - first : nt * kBM;
        const dim3 grid((u32)(nt * g.nct));
        if (vec) hipLaunchKernelGGL((mlp_infer_gemm_kernel<WIDE, true>), grid, dim3(kBlock), 0, st, c);
        else hipLaunchKernelGGL((mlp_infer_gemm_kernel<WIDE, false>), grid, dim3(kBlock), 0, st, c);
        if (const int rc = launch_status("mlp_infer_gemm_kernel")) return rc;
    }
    return GP_OK;
}

}  // namespace

extern "C" {

int gp_mlp_infer_block(int device, const float* d_x, int64_t n_rows, int32_t f_in, int32_t f_out,
                       const float* d_weight, const float* d_bias, int flags,
                       const float* d_bn_weight, const float* d_bn_bias,
                       const float* d_running_mean, const float* d_running_var, float bn_eps,
                       float* d_out, void* d_workspace, void* stream)
{
    const char* where = "gp_mlp_infer_block";
    const bool norm = (flags & GP_MLP_NORM) != 0, bn = (flags & GP_MLP_BN) != 0;
    if (n_rows < 0 || f_in < 1 || f_out < 1 || (flags & ~(GP_MLP_RELU | GP_MLP_NORM | GP_MLP_BN)))
        return fail(GP_ERR_INVALID_ARG, where, "n_rows < 0, f_in < 1, f_out < 1, or a flag other than GP_MLP_RELU, GP_MLP_NORM and "
                                               "GP_MLP_BN (inference has no training mode)");
    if (n_rows > (1ll << 40) || (long long)f_in * f_out > (1ll << 40) || f_out > (1 << 22))
        return fail(GP_ERR_INVALID_ARG, where, "sizes out of range");
    if (bn && !(bn_eps > 0.0f)) return fail(GP_ERR_INVALID_ARG, where, "bn_eps <= 0");
    if (n_rows == 0) return GP_OK;
    if (!d_x || !d_weight || !d_out || ((norm || bn) && !d_workspace) || (bn && (!d_running_mean || !d_running_var)))
        return fail(GP_ERR_NULL, where, "a device pointer is NULL");
    if (const int rc = set_device(device, where)) return rc;
    hipStream_t st = (hipStream_t)stream;
    float* ws = static_cast<float*>(d_workspace);                    // [n_rows] row scales, [f_in] mul, [f_in] add
    Infer g = {};
    g.x = d_x; g.M = n_rows; g.K = f_in; g.N = f_out;
    g.w = d_weight; g.bias = d_bias; g.y = d_out;
    g.relu = (flags & GP_MLP_RELU) != 0;
    if (norm) {
        g.r = ws;
        if (const int rc = launch_row_scales(d_x, n_rows, f_in, g.relu, ws, st)) return rc;
    }
    if (bn) {
        g.mul = ws + n_rows; g.add = ws + n_rows + f_in;
        if (const int rc = launch_bn_fold(f_in, d_bn_weight, d_bn_bias, d_running_mean, d_running_var, bn_eps, ws + n_rows, st)) return rc;
    }
    return f_out > 64 ? run_gemm<true>(g, st) : run_gemm<false>(g, st);
}

}  // extern "C"
