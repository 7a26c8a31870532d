/*
 * grandplus_infer.h -- the inference entry point of the C ABI (implemented by grand_plus_amd/csrc/mlp_infer.hip).
 *
 * Part of the ABI that grandplus.h describes (GP_ABI_VERSION, the status codes and the GP_MLP_* flags are defined
 * there): grandplus.h includes this file, so callers include grandplus.h alone.  The ctypes binding declares the entry
 * point under this file's name in _native.ABI, and tests/test_host_abi.py holds that table against this file type by type.
 */
#ifndef GRANDPLUS_INFER_H
#define GRANDPLUS_INFER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * One MLP block in eval mode over any number of rows (the reference's get_local_logits, model.py:169-178,
 * pushes every node of the graph through the MLP in eval mode):
 *
 *     y = Linear( BN_running( node_norm( relu?(x) ) ) ),      node_norm(u) = u / (1e-12 + |u|_2)
 *
 * d_x fp32 [n_rows x f_in] and d_out fp32 [n_rows x f_out] row-major and dense; d_x needs 4-byte alignment only (a row
 * slice of a larger tensor is fine: 16-byte loads are used where the pointers and f_in allow them, the same arithmetic
 * otherwise).  d_weight [f_out x f_in] and d_bias [f_out] (NULL = no bias) as nn.Linear holds them.  flags: GP_MLP_RELU,
 * GP_MLP_NORM, GP_MLP_BN and nothing else: there is no training mode, no dropout and no sample dimension.  With
 * GP_MLP_BN the running statistics d_running_mean / d_running_var [f_in] are required and only read; d_bn_weight /
 * d_bn_bias [f_in] may be NULL (1 and 0).  d_workspace: GP_MLP_INFER_WORKSPACE_BYTES(n_rows, f_in) bytes of device
 * memory, 4-byte aligned, the caller's; it may be NULL when neither GP_MLP_NORM nor GP_MLP_BN is set.
 *
 * At most three launches: the row scales (GP_MLP_NORM), the BatchNorm fold (GP_MLP_BN), the GEMM (a 128 x 128 tile on
 * v_mfma_f32_32x32x2_f32 for f_out > 64, a 128 x 64 tile on v_mfma_f32_16x16x4_f32 otherwise; more than 2^29 rows are
 * cut into several GEMM launches).
 *
 * Contracts:
 *   - arithmetic: fp32 throughout, exact-fp32 MFMA, no contraction.  With a = (relu?(x) * r_m) * mul_k + add_k,
 *         acc = +0;  for k = 0 ... f_in - 1 ascending: acc = fma(a[m,k], W[n,k], acc);  y[m,n] = acc + b[n]
 *     one chain per output, whatever the tile, n_rows or f_out (the k tail up to the next multiple of 16 adds
 *     fma(0, 0, acc)).  r_m = 1 / (1e-12 + sqrt(sum_k u^2)) with lane l of a wave summing k = l, l + 64, ... and then the
 *     wave butterfly; mul_k = gamma_k * is_k, add_k = beta_k - mean_k * (gamma_k * is_k), is_k = 1 / sqrt(var_k + eps):
 *     the arithmetic and order of gp_mlp_block_forward in eval mode, so both give the same bits wherever that one takes
 *     a single k-chain (f_in <= 64, or at least 128 tiles of 64 x 64);
 *   - row independence: output row m depends on input row m and the parameters only, so any split of the rows into
 *     calls gives the same bits; a NaN in input row m stays a NaN through GP_MLP_RELU (torch's relu, not fmaxf), so a
 *     chain of layers hands it on to output row m and to no other row;
 *   - no atomics;
 *   - nothing on the call path synchronises, copies or allocates; every launch is enqueued on `stream`;
 *   - n_rows == 0 is GP_OK with nothing launched (the pointers are not looked at);
 *   - arguments are checked before the device is touched: GP_ERR_INVALID_ARG for n_rows < 0, f_in < 1, f_out < 1,
 *     n_rows > 2^40, f_in * f_out > 2^40, f_out > 2^22, any flag outside the three (GP_MLP_TRAINING included), or
 *     bn_eps <= 0 with GP_MLP_BN; GP_ERR_NULL for a missing pointer (d_x, d_weight, d_out; the running statistics with
 *     GP_MLP_BN; the workspace with GP_MLP_NORM or GP_MLP_BN).
 * ------------------------------------------------------------------------------------------ */
#define GP_MLP_INFER_WORKSPACE_BYTES(n_rows, f_in) ((4 * ((int64_t)(n_rows) + 2 * (int64_t)(f_in)) + 15) / 16 * 16)

int gp_mlp_infer_block(int device, const float* d_x, int64_t n_rows, int32_t f_in, int32_t f_out,
                       const float* d_weight, const float* d_bias, int flags,
                       const float* d_bn_weight, const float* d_bn_bias,
                       const float* d_running_mean, const float* d_running_var, float bn_eps,
                       float* d_out, void* d_workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GRANDPLUS_INFER_H */
