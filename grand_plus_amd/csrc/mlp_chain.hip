// mlp_chain.hip -- the last two eval blocks of the MLP as one kernel (gp_mlp_infer_chain2 of
// grandplus_infer_chain.h).  A workgroup owns BM rows and keeps their hidden activations in LDS:
//
//     y1[BM x H] = a1 W1^T + b1        a1 = (relu?(x) * r1_m) * mul1_k + add1_k         -> the LDS hidden tile
//     r2_m       = 1 / (1e-12 + |relu?(y1_m)|_2)                                        from the tile
//     out[BM x C] = a2 W2^T + b2       a2 = (relu?(y1) * r2_m) * mul2_k + add2_k        applied as the tile is read
//
//   mlp_eval_row_kernel    r1                                                                   (GP_MLP_NORM of block 1)
//   mlp_eval_fold_kernel   mul / add                                                            (GP_MLP_BN, once per block)
//   mlp_chain_kernel       the three steps above; BM = 128 (H <= 128), 64 (H <= 512), 32 (H <= 1024)
//
// Arithmetic contract: the bits of gp_mlp_infer_block for block 1 into a [n_rows x H] buffer followed by
// gp_mlp_infer_block for block 2.  Both units take every formula from mlp_eval.hpp: the prologue, the row sum (r2 through
// row_inv_norm, over the tile), the fold and the NaN-keeping relu.  The k tail up to the next
// multiple of 16 adds fma(0, 0, acc) as there, and r2 is NOT pulled out of the second product.  No atomics.
//
// Block 1 loops over chunks of 128 hidden columns and, inside a chunk, over k in stages of 16 through two LDS stages
// (mlp_infer.hip's pipeline and LDS image: rows 20 floats apart, the k of a row permuted when written so that one
// ds_read_b128 hands a lane its k of four MFMA steps); the x tile is read again from L2 for every chunk.  Its MFMA is
// v_mfma_f32_32x32x2_f32.  A hidden value y1[m, k] is stored at row m, position (k & ~15) + kperm16(k & 15) of the tile,
// kperm16 being the permutation of the 16x16x4 operand: block 2 (v_mfma_f32_16x16x4_f32, 32 k per stage of W2, mul2 and
// add2) reads its A operand from the tile with one ds_read_b128 per 16 k.  k of one output is never split across waves:
// the waves share the output fragments.
#include "mlp_eval.hpp"

namespace {

constexpr int kCN = 128;              // hidden columns per chunk of block 1
constexpr int kSub = 2;               // block 2: 16-deep sub-stages per stage
constexpr int kSubRows = GP_MLP_CHAIN_MAX_OUT + 2;   // W2's rows, then mul2 and add2

struct Chain {
    const float* x; long long M; int K; int H; int C;
    const float* w1; const float* b1; int relu1;
    const float* r1;                      // [M] row scales of x, or NULL
    const float* mul1; const float* add1; // [K] folded BatchNorm of block 1, or NULL
    const float* w2; const float* b2; int relu2; int norm2;
    const float* mul2; const float* add2; // [H] folded BatchNorm of block 2, or NULL
    float* out;
    int hs;                               // floats between the rows of the hidden tile
};

// where hidden column k is stored in its row of the tile: block 2's A operand, permuted when written
__device__ __forceinline__ int hid_pos(int k) { return (k & ~15) + kperm16(k & 15); }

constexpr int chain_stage_floats(int BM) { return (BM + kCN) * kStride; }
constexpr int chain_lds_floats(int BM, int hs) { return BM * hs + BM + 2 * chain_stage_floats(BM); }

template <int BM, bool VEC1, bool VEC2>
__global__ void __launch_bounds__(kBlock)
mlp_chain_kernel(Chain g)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int STG = chain_stage_floats(BM);
    static_assert(kSub * kSubRows * kStride <= STG, "block 2's stage fits block 1's");
    float* hid = lds;                                 // [BM][hs]
    float* r2 = hid + BM * g.hs;                      // [BM]
    float* stg = r2 + BM;                             // [2][STG]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long m0 = (long long)blockIdx.x * BM;
    const int K = g.K, H = g.H, C = g.C, hs = g.hs;

    // ------------------------------------------------------------------------------------------------ block 1
    {
        constexpr int NA = (BM * 4 + kBlock - 1) / kBlock, NW = kCN * 4 / kBlock;   // quads of 4 k per thread and stage
        constexpr int WR = BM >= 64 ? 2 : 1, WC = 4 / WR;                           // the wave grid over a BM x 128 chunk
        constexpr int FI = BM / WR / 32, FJ = kCN / WC / 32;                        // 32 x 32 fragments per wave
        const int fl = lane & 31, fh = lane >> 5;
        const int wr = (wave % WR) * (BM / WR), wc = (wave / WR) * (kCN / WC);
        int ar[NA], ak[NA]; bool a_ok[NA]; const float* ap[NA]; float rm[NA];
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int q = t + kBlock * i;
            ar[i] = q >> 2; ak[i] = (q & 3) * 4;
            const long long am = m0 + ar[i];
            a_ok[i] = q < BM * 4 && am < g.M;
            ap[i] = g.x + (a_ok[i] ? am : 0) * K;
            rm[i] = (g.r1 && a_ok[i]) ? g.r1[am] : 1.0f;
        }
        const int nst = (K + kBK - 1) / kBK;
        for (int n0 = 0; n0 < H; n0 += kCN) {
            int br[NW], bk[NW]; bool b_ok[NW]; const float* bp[NW];
#pragma unroll
            for (int i = 0; i < NW; ++i) {
                const int q = t + kBlock * i;
                br[i] = q >> 2; bk[i] = (q & 3) * 4;
                b_ok[i] = n0 + br[i] < H;
                bp[i] = g.w1 + (long long)(b_ok[i] ? n0 + br[i] : 0) * K;
            }
            float xa[NA][4], mu[NA][4], ad[NA][4], wb[NW][4];
            auto load = [&](int k0) {
#pragma unroll
                for (int i = 0; i < NA; ++i) {
                    if (BM * 4 < kBlock && t >= BM * 4) continue;
                    load_row<4, VEC1>(ap[i], a_ok[i], k0 + ak[i], K, xa[i]);
                    if (g.mul1) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const bool ok = k0 + ak[i] + j < K;
                            mu[i][j] = ok ? g.mul1[k0 + ak[i] + j] : 0.0f;
                            ad[i][j] = ok ? g.add1[k0 + ak[i] + j] : 0.0f;
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < NW; ++i) load_row<4, VEC1>(bp[i], b_ok[i], k0 + bk[i], K, wb[i]);
            };
            auto stage = [&](int k0, float* buf) {
#pragma unroll
                for (int i = 0; i < NA; ++i) {
                    if (BM * 4 < kBlock && t >= BM * 4) continue;
                    float* arow = buf + ar[i] * kStride;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool ok = a_ok[i] && k0 + ak[i] + j < K;
                        const float v = ok ? eval_prologue(xa[i][j], g.relu1, g.r1, rm[i], g.mul1, mu[i][j], ad[i][j]) : 0.0f;
                        arow[kperm32(ak[i] + j)] = v;
                    }
                }
#pragma unroll
                for (int i = 0; i < NW; ++i) {
                    float* brow = buf + (BM + br[i]) * kStride;
#pragma unroll
                    for (int j = 0; j < 4; ++j) brow[kperm32(bk[i] + j)] = wb[i][j];
                }
            };

            f32x16 acc[FI][FJ];
#pragma unroll
            for (int i = 0; i < FI; ++i)
#pragma unroll
                for (int j = 0; j < FJ; ++j)
#pragma unroll
                    for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.0f;
            bool jact[FJ];                                   // a column fragment with no hidden column is skipped (wave-uniform)
#pragma unroll
            for (int j = 0; j < FJ; ++j) jact[j] = n0 + wc + j * 32 < H;

            load(0);
            stage(0, stg);
            __syncthreads();
            for (int s = 0; s < nst; ++s) {
                const float* buf = stg + (s & 1) * STG;
                if (s + 1 < nst) load((s + 1) * kBK);
                float a[FI][8], b[FJ][8];
#pragma unroll
                for (int i = 0; i < FI; ++i)
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const f32x4 v = *reinterpret_cast<const f32x4*>(buf + (wr + i * 32 + fl) * kStride + fh * 8 + 4 * q);
#pragma unroll
                        for (int e = 0; e < 4; ++e) a[i][4 * q + e] = v[e];
                    }
#pragma unroll
                for (int j = 0; j < FJ; ++j)
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const f32x4 v = *reinterpret_cast<const f32x4*>(buf + (BM + wc + j * 32 + fl) * kStride + fh * 8 + 4 * q);
#pragma unroll
                        for (int e = 0; e < 4; ++e) b[j][4 * q + e] = v[e];
                    }
#pragma unroll
                for (int ks = 0; ks < 8; ++ks)
#pragma unroll
                    for (int i = 0; i < FI; ++i)
#pragma unroll
                        for (int j = 0; j < FJ; ++j)
                            if (jact[j]) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][ks], b[j][ks], acc[i][j], 0, 0, 0);
                if (s + 1 < nst) stage((s + 1) * kBK, stg + ((s + 1) & 1) * STG);
                __syncthreads();
            }

            // C/D of 32x32: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5); y1 = acc + b1 into the tile
#pragma unroll
            for (int i = 0; i < FI; ++i)
#pragma unroll
                for (int j = 0; j < FJ; ++j) {
                    const int col = n0 + wc + j * 32 + fl;
                    if (col >= H) continue;
                    const float bv = g.b1 ? g.b1[col] : 0.0f;
                    const int pos = hid_pos(col);
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const int row = wr + i * 32 + (q & 3) + 8 * (q >> 2) + 4 * fh;
                        float v = acc[i][j][q];
                        if (g.b1) v = v + bv;
                        hid[row * hs + pos] = v;
                    }
                }
        }
    }
    __syncthreads();

    // -------------------------------------------------------------------------- r2: the row sum of mlp_eval.hpp, from the tile
    if (g.norm2) {
        for (int row = wave; row < BM; row += kBlock / 64) {
            const float* hr = hid + row * hs;
            const float rm = row_inv_norm(H, lane, [&](int k) { return g.relu2 ? relu_nan(hr[hid_pos(k)]) : hr[hid_pos(k)]; });
            if (lane == 0) r2[row] = rm;
        }
    }
    // (the barrier after stage 0 of block 2 orders r2 before its first read)

    // ------------------------------------------------------------------------------------------------ block 2
    {
        constexpr int RF = BM / 16;                          // row fragments of the tile
        constexpr int RPW = BM >= 128 ? 2 : 1;               // row fragments per wave
        constexpr int WRG = RF / RPW, WCG = 4 / WRG;         // wave groups over rows and over column fragments
        constexpr int CPW = 4 / WCG;                         // column fragments per wave
        constexpr int SUBF = kSubRows * kStride;             // floats of a sub-stage
        constexpr int NQ = GP_MLP_CHAIN_MAX_OUT * kSub * 4 / kBlock;   // W2 quads per thread and stage
        const int fl = lane & 15, fh = lane >> 4;
        const int wrg = wave % WRG, wcg = wave / WRG;
        const int nfrag = (C + 15) / 16;
        int br[NQ], kq[NQ]; bool b_ok[NQ]; const float* bp[NQ];
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int q = t + kBlock * i;
            br[i] = q / (kSub * 4); kq[i] = (q % (kSub * 4)) * 4;
            b_ok[i] = br[i] < C;
            bp[i] = g.w2 + (long long)(b_ok[i] ? br[i] : 0) * H;
        }
        float wb[NQ][4], ma = 0.0f;
        auto load = [&](int k0) {
#pragma unroll
            for (int i = 0; i < NQ; ++i) load_row<4, VEC2>(bp[i], b_ok[i], k0 + kq[i], H, wb[i]);
            if (t < 64) {                                    // mul2 (t < 32) and add2 of this stage's 32 k
                const int k = k0 + (t & 31);
                ma = (g.mul2 && k < H) ? (t < 32 ? g.mul2[k] : g.add2[k]) : 0.0f;
            }
        };
        auto stage = [&](float* buf) {
#pragma unroll
            for (int i = 0; i < NQ; ++i) {
                float* brow = buf + (kq[i] >> 4) * SUBF + br[i] * kStride;
#pragma unroll
                for (int j = 0; j < 4; ++j) brow[kperm16((kq[i] & 15) + j)] = wb[i][j];
            }
            if (t < 64) buf[((t & 31) >> 4) * SUBF + (GP_MLP_CHAIN_MAX_OUT + (t >> 5)) * kStride + kperm16(t & 15)] = ma;
        };

        f32x4 acc[RPW][CPW];
#pragma unroll
        for (int i = 0; i < RPW; ++i)
#pragma unroll
            for (int j = 0; j < CPW; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

        const int nst = (H + kSub * kBK - 1) / (kSub * kBK);
        load(0);
        stage(stg);
        __syncthreads();
        float rmv[RPW];
#pragma unroll
        for (int i = 0; i < RPW; ++i) rmv[i] = g.norm2 ? r2[(wrg * RPW + i) * 16 + fl] : 1.0f;
        for (int s = 0; s < nst; ++s) {
            const float* buf = stg + (s & 1) * STG;
            const int k0 = s * kSub * kBK;
            if (s + 1 < nst) load(k0 + kSub * kBK);
#pragma unroll
            for (int sub = 0; sub < kSub; ++sub) {
                const int ks = k0 + sub * kBK;               // the 16 k of this sub-stage: a lane holds ks + fh + 4 e of step e
                if (ks >= H) continue;                       // the unfused GEMM has no such stage either
                const float* sb = buf + sub * SUBF;
                float a[RPW][4];
                const f32x4 mu = *reinterpret_cast<const f32x4*>(sb + GP_MLP_CHAIN_MAX_OUT * kStride + 4 * fh);
                const f32x4 ad = *reinterpret_cast<const f32x4*>(sb + (GP_MLP_CHAIN_MAX_OUT + 1) * kStride + 4 * fh);
#pragma unroll
                for (int i = 0; i < RPW; ++i) {
                    const f32x4 y = *reinterpret_cast<const f32x4*>(hid + ((wrg * RPW + i) * 16 + fl) * hs + ks + 4 * fh);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float v = eval_prologue(y[e], g.relu2, g.norm2, rmv[i], g.mul2, mu[e], ad[e]);
                        a[i][e] = ks + fh + 4 * e < H ? v : 0.0f;
                    }
                }
#pragma unroll
                for (int j = 0; j < CPW; ++j) {
                    const int cf = wcg * CPW + j;
                    if (cf >= nfrag) continue;
                    const f32x4 b = *reinterpret_cast<const f32x4*>(sb + (cf * 16 + fl) * kStride + 4 * fh);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int i = 0; i < RPW; ++i)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][e], b[e], acc[i][j], 0, 0, 0);
                }
            }
            if (s + 1 < nst) stage(stg + ((s + 1) & 1) * STG);
            __syncthreads();
        }

        // C/D of 16x16: col = lane & 15, row = 4 (lane >> 4) + reg
#pragma unroll
        for (int i = 0; i < RPW; ++i)
#pragma unroll
            for (int j = 0; j < CPW; ++j) {
                const int col = (wcg * CPW + j) * 16 + fl;
                if (col >= C) continue;
                const float bv = g.b2 ? g.b2[col] : 0.0f;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const long long row = m0 + (wrg * RPW + i) * 16 + 4 * fh + q;
                    if (row >= g.M) continue;
                    float v = acc[i][j][q];
                    if (g.b2) v = v + bv;
                    g.out[row * C + col] = v;
                }
            }
    }
}

// ---- host side
typedef void (*ChainKernel)(Chain);

template <int BM>
ChainKernel pick(bool v1, bool v2)
{
    return v1 ? (v2 ? mlp_chain_kernel<BM, true, true> : mlp_chain_kernel<BM, true, false>)
              : (v2 ? mlp_chain_kernel<BM, false, true> : mlp_chain_kernel<BM, false, false>);
}

int run_chain(Chain g, hipStream_t st)
{
    // rows per workgroup follow H: the hidden tile and two stages have to fit 160 KB of LDS
    const int BM = g.H <= 128 ? 128 : g.H <= 512 ? 64 : 32;
    g.hs = (g.H + 15) / 16 * 16 + 4;
    const int lds_bytes = 4 * chain_lds_floats(BM, g.hs);
    // float4 loads need 16-byte row starts in both operands of a block
    const bool v1 = (g.K & 3) == 0 && (((uintptr_t)g.x | (uintptr_t)g.w1) & 15) == 0;
    const bool v2 = (g.H & 3) == 0 && ((uintptr_t)g.w2 & 15) == 0;
    const ChainKernel k = BM == 128 ? pick<128>(v1, v2) : BM == 64 ? pick<64>(v1, v2) : pick<32>(v1, v2);
    // the limit is the instantiation's own maximum (the largest H its BM serves), not this call's size: whatever order
    // host threads call in, no call lowers the limit under another one's launch
    const int max_h = BM == 128 ? 128 : BM == 64 ? 512 : GP_MLP_CHAIN_MAX_HIDDEN;
    const int lds_limit = 4 * chain_lds_floats(BM, max_h + 4);
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, lds_limit) != hipSuccess)
        return launch_status("mlp_chain_kernel (LDS size)");
    const long long row_tiles = cdiv(g.M, BM);
    for (long long t0 = 0; t0 < row_tiles; t0 += kMaxGrid) {               // one launch unless there are more than 2^22 tiles
        const long long nt = row_tiles - t0 < kMaxGrid ? row_tiles - t0 : kMaxGrid;
        Chain c = g;
        const long long first = t0 * BM;
        c.x = g.x + first * g.K; c.out = g.out + first * g.C; c.r1 = g.r1 ? g.r1 + first : nullptr;
        c.M = g.M - first < nt * BM ? g.M - first : nt * BM;
        hipLaunchKernelGGL(k, dim3((u32)nt), dim3(kBlock), (size_t)lds_bytes, st, c);
        if (const int rc = launch_status("mlp_chain_kernel")) return rc;
    }
    return GP_OK;
}

}  // namespace

extern "C" {

int gp_mlp_infer_chain2(int device, const float* d_x, int64_t n_rows, int32_t f_in, int32_t f_hidden, int32_t f_out,
                        const float* d_w1, const float* d_b1, int flags1, const float* d_bn1_weight, const float* d_bn1_bias,
                        const float* d_bn1_mean, const float* d_bn1_var, float bn1_eps,
                        const float* d_w2, const float* d_b2, int flags2, const float* d_bn2_weight, const float* d_bn2_bias,
                        const float* d_bn2_mean, const float* d_bn2_var, float bn2_eps,
                        float* d_out, void* d_workspace, void* stream)
{
    const char* where = "gp_mlp_infer_chain2";
    const int known = GP_MLP_RELU | GP_MLP_NORM | GP_MLP_BN;
    const bool norm1 = (flags1 & GP_MLP_NORM) != 0, bn1 = (flags1 & GP_MLP_BN) != 0;
    const bool norm2 = (flags2 & GP_MLP_NORM) != 0, bn2 = (flags2 & GP_MLP_BN) != 0;
    if (n_rows < 0 || f_in < 1 || f_hidden < 1 || f_out < 1 || (flags1 & ~known) || (flags2 & ~known))
        return fail(GP_ERR_INVALID_ARG, where, "n_rows < 0, f_in < 1, f_hidden < 1, f_out < 1, or a flag other than GP_MLP_RELU, "
                                               "GP_MLP_NORM and GP_MLP_BN (inference has no training mode)");
    if (f_hidden > GP_MLP_CHAIN_MAX_HIDDEN || f_out > GP_MLP_CHAIN_MAX_OUT)
        return fail(GP_ERR_INVALID_ARG, where, "f_hidden > 1024 or f_out > 64: the hidden tile has to fit a workgroup's LDS");
    if (n_rows > (1ll << 40) || (long long)f_in * f_hidden > (1ll << 40) || f_in > INT32_MAX - 31)
        return fail(GP_ERR_INVALID_ARG, where, "sizes out of range");      // f_in + 31 stays an int: the k of a padded stage
    if ((bn1 && !(bn1_eps > 0.0f)) || (bn2 && !(bn2_eps > 0.0f))) return fail(GP_ERR_INVALID_ARG, where, "bn_eps <= 0");
    if (n_rows == 0) return GP_OK;
    if (!d_x || !d_w1 || !d_w2 || !d_out || ((norm1 || bn1 || norm2 || bn2) && !d_workspace) ||
        (bn1 && (!d_bn1_mean || !d_bn1_var)) || (bn2 && (!d_bn2_mean || !d_bn2_var)))
        return fail(GP_ERR_NULL, where, "a device pointer is NULL");
    if (const int rc = set_device(device, where)) return rc;
    hipStream_t st = (hipStream_t)stream;
    float* ws = static_cast<float*>(d_workspace);    // [n_rows] row scales of x, [f_in] mul1, [f_in] add1, [f_hidden] mul2, add2
    Chain g = {};
    g.x = d_x; g.M = n_rows; g.K = f_in; g.H = f_hidden; g.C = f_out;
    g.w1 = d_w1; g.b1 = d_b1; g.relu1 = (flags1 & GP_MLP_RELU) != 0;
    g.w2 = d_w2; g.b2 = d_b2; g.relu2 = (flags2 & GP_MLP_RELU) != 0; g.norm2 = norm2;
    g.out = d_out;
    if (norm1) {
        g.r1 = ws;
        if (const int rc = launch_row_scales(d_x, n_rows, f_in, g.relu1, ws, st)) return rc;
    }
    if (bn1) {
        float* mul = ws + n_rows;
        g.mul1 = mul; g.add1 = mul + f_in;
        if (const int rc = launch_bn_fold(f_in, d_bn1_weight, d_bn1_bias, d_bn1_mean, d_bn1_var, bn1_eps, mul, st)) return rc;
    }
    if (bn2) {
        float* mul = ws + n_rows + 2ll * f_in;
        g.mul2 = mul; g.add2 = mul + f_hidden;
        if (const int rc = launch_bn_fold(f_hidden, d_bn2_weight, d_bn2_bias, d_bn2_mean, d_bn2_var, bn2_eps, mul, st)) return rc;
    }
    return run_chain(g, st);
}

}  // extern "C"
