// mag_stage.hpp -- what MAG's kernels share besides dropnode.hpp: the operands of a call (MagArgs), the staging of one
// resident row's columns and DropNode weights in LDS, the workgroup shape and the entry points' argument check.
// mag_prop.hip (§7k: the forward and the atomic backward) and mag_det.hip (§7o: the deterministic backward) call these
// lines, so a slot is present, weighted and masked in the backward exactly as the forward had it; row_mark.hip (§7u)
// finds a slot's node by mag_det.hip's rule.  Everything has internal linkage, as in gp_common.hpp.
#pragma once

#include "dropnode.hpp"

namespace {

constexpr int kMaxWaves = 16;
constexpr int kLdsFloats = 65536 / 4;
constexpr int kGridCap = 8192;                         // workgroups of up to 1 024 threads: 32 per CU on 256 CUs

struct MagArgs {
    long long V; int H;
    const long long* indptr; const int* indices; const float* data; long long N;
    const int* col; const double* val; const int* filled; long long n_rows; int K;
    const int* batch_rows; int B; int S; int nsc;
    float p_node, p_in; int training; u64 seed;
    const unsigned char* keep; long long keep_stride;
    const u64* d_seed;                                   // the seed in device memory; null: `seed` above
};

// The seed of a call: read once by every kernel, before its row loop; the DropNode hash (stage_row) and the input dropout's
// slot seeds derive from this value alone.  A captured graph freezes the pointer, not the value behind it.
__device__ __forceinline__ u64 call_seed(const MagArgs& A) { return A.d_seed ? *A.d_seed : A.seed; }

// what finds a slot's node without the weights: the attribute CSR's row pointers, the resident rows and the batch
// (mag_det.hip's key kernels and gather, row_mark.hip's mark kernel)
struct SlotArgs {
    const long long* indptr; const int* indices; long long N, V;
    const int* col; const int* filled; long long n_rows; int K;
    const int* batch_rows;
};

// whether slot e = b * K + k exists (mag_det_abi.hpp), and its node
__device__ __forceinline__ bool slot_node(const SlotArgs& A, long long e, long long& node)
{
    const long long b = e / A.K;
    const int k = (int)(e - b * A.K);
    const long long row = A.batch_rows ? (long long)A.batch_rows[b] : b;
    node = 0;
    if (row < 0 || row >= A.n_rows || k >= row_len(A.filled, row, A.K)) return false;
    node = A.col[row * (long long)A.K + k];
    return node >= 0 && node < A.N;
}

// Stage the row's columns (first chunk) and the weights of samples s0 .. s0 + ns - 1; a column outside [0, N) makes
// the slot absent (weight 0).  seed: call_seed(A).  Called by every thread, between two barriers of the caller.
__device__ __forceinline__ void stage_row(const MagArgs& A, u64 seed, long long row, int n, int s0, int ns, float scale_node,
                                          int* s_col, int* s_seen, float* s_w, int* n_bad)
{
    for (int k = threadIdx.x; k < n; k += blockDim.x) {
        const long long e = row * (long long)A.K + k;
        const float w = (float)A.val[e];                              // model_mag.py:343
        const int c = A.col[e];
        const bool c_ok = c >= 0 && c < A.N;
        if (s0 == 0) {
            s_col[k] = c;
            if (s_seen) s_seen[k] = 0;
            if (!c_ok && n_bad) atomicAdd(n_bad, 1);
        }
        for (int s = 0; s < ns; ++s)
            s_w[s * A.K + k] = c_ok ? sample_weight(w, e, s0 + s, A.p_node, scale_node, A.training, seed, A.keep, A.keep_stride) : 0.0f;
    }
}

int mag_check(const char* where, int64_t n_vocab, int32_t dim, int64_t n_nodes, int64_t n_rows, int32_t K, int32_t n_batch,
              int32_t n_samples, float p_node, float p_in, const void* keep, int64_t keep_stride)
{
    if (n_samples < 1 || n_samples > kMaxSamples || !(p_node >= 0.0f && p_node <= 1.0f) || !(p_in >= 0.0f && p_in <= 1.0f))
        return fail(GP_ERR_INVALID_ARG, where, "n_samples outside [1, 16] or a rate outside [0, 1]");
    if (n_vocab < 1 || dim < 1 || n_nodes < 0 || n_rows < 0 || K < 1 || K > GP_MAX_K || n_batch < 0 || (keep && keep_stride < 1))
        return fail(GP_ERR_INVALID_ARG, where, "bad size, K outside [1, 1024] or keep_stride < 1 with a mask");
    return GP_OK;
}

int waves_for(int K)                                   // min(16, the power of two >= K): a function of K alone
{
    int w = 1;
    while (w < K && w < kMaxWaves) w <<= 1;
    return w;
}

}  // namespace
