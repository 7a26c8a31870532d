/*
 * grandplus_infer_chain.h -- the fused two-block inference entry point of the C ABI (implemented by
 * grand_plus_amd/csrc/mlp_chain.hip).
 *
 * Part of the ABI that grandplus.h describes (GP_ABI_VERSION, the status codes and the GP_MLP_* flags are defined
 * there): grandplus.h includes this file, so callers include grandplus.h alone.  The ctypes binding declares the entry
 * point under this file's name in _native.ABI, and tests/test_host_abi.py holds that table against this file type by type.
 */
#ifndef GRANDPLUS_INFER_CHAIN_H
#define GRANDPLUS_INFER_CHAIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Two consecutive MLP blocks in eval mode as one kernel: the last two blocks of every two-block layout,
 *
 *     y1  = Linear1( BN1_running( node_norm( relu?(x) ) ) )          [n_rows x f_hidden], kept in LDS, never in memory
 *     out = Linear2( BN2_running( node_norm( relu?(y1) ) ) )         [n_rows x f_out]
 *
 * One workgroup owns a tile of rows (128 for f_hidden <= 128, 64 up to 512, 32 up to 1024), computes their hidden
 * activations into LDS, takes block 2's row scales from there and multiplies by W2 out of LDS.
 *
 * Each block's arguments are gp_mlp_infer_block's (grandplus_infer.h): d_x fp32 [n_rows x f_in] row-major and dense,
 * 4-byte aligned (16-byte loads are used where the pointers and the widths allow them, the same arithmetic otherwise);
 * d_w1 [f_hidden x f_in], d_b1 [f_hidden], d_w2 [f_out x f_hidden], d_b2 [f_out] as nn.Linear holds them (a NULL bias =
 * none); flags1 / flags2: GP_MLP_RELU, GP_MLP_NORM, GP_MLP_BN and nothing else; with GP_MLP_BN the block's running
 * statistics ([f_in] for block 1, [f_hidden] for block 2) are required and only read, its weight / bias may be NULL
 * (1 and 0).  d_workspace: GP_MLP_INFER_CHAIN_WORKSPACE_BYTES(n_rows, f_in, f_hidden) bytes of device memory, 4-byte
 * aligned, the caller's; it may be NULL when neither block sets GP_MLP_NORM or GP_MLP_BN.
 *
 * At most four launches: the row scales of x (GP_MLP_NORM of block 1), one BatchNorm fold per block with GP_MLP_BN, the
 * chain kernel (more than 2^22 row tiles are cut into several launches of it).
 *
 * Contracts:
 *   - the result equals gp_mlp_infer_block for block 1 into a [n_rows x f_hidden] buffer followed by
 *     gp_mlp_infer_block for block 2, BIT FOR BIT, for every shape, flag set, alignment and n_rows: the same k-chains in
 *     the same order (acc = +0; k ascending: acc = fma(a, W, acc); + b; the k tail up to the next multiple of 16 adds
 *     fma(0, 0, acc)), the same row-scale summation order (lane l of a wave sums k = l, l + 64, ..., then the wave
 *     butterfly), the same BatchNorm fold and the same NaN-keeping relu; block 2's row scale is applied to each hidden
 *     value before the product, never pulled out of it.  Row independence and NaN containment (a NaN in input row m
 *     makes output row m NaN and touches no other row) follow;
 *   - no atomics;
 *   - nothing on the call path synchronises, copies or allocates; every launch is enqueued on `stream`;
 *   - n_rows == 0 is GP_OK with nothing launched (the pointers are not looked at);
 *   - arguments are checked before the device is touched: GP_ERR_INVALID_ARG for n_rows < 0, f_in < 1, f_hidden < 1,
 *     f_out < 1, f_hidden > GP_MLP_CHAIN_MAX_HIDDEN, f_out > GP_MLP_CHAIN_MAX_OUT, n_rows > 2^40,
 *     f_in * f_hidden > 2^40, f_in > 2^31 - 32, any flag outside the three in either block (GP_MLP_TRAINING
 *     included), or a block's bn_eps <= 0 with its GP_MLP_BN; GP_ERR_NULL for a missing pointer (d_x, d_w1, d_w2, d_out; a block's running
 *     statistics with its GP_MLP_BN; the workspace with GP_MLP_NORM or GP_MLP_BN in either block).
 * ------------------------------------------------------------------------------------------ */
#define GP_MLP_CHAIN_MAX_HIDDEN 1024
#define GP_MLP_CHAIN_MAX_OUT 64
#define GP_MLP_INFER_CHAIN_WORKSPACE_BYTES(n_rows, f_in, f_hidden) ((4 * ((int64_t)(n_rows) + 2 * (int64_t)(f_in) + 2 * (int64_t)(f_hidden)) + 15) / 16 * 16)

int gp_mlp_infer_chain2(int device, const float* d_x, int64_t n_rows, int32_t f_in, int32_t f_hidden, int32_t f_out,
                        const float* d_w1, const float* d_b1, int flags1, const float* d_bn1_weight, const float* d_bn1_bias,
                        const float* d_bn1_mean, const float* d_bn1_var, float bn1_eps,
                        const float* d_w2, const float* d_b2, int flags2, const float* d_bn2_weight, const float* d_bn2_bias,
                        const float* d_bn2_mean, const float* d_bn2_var, float bn2_eps,
                        float* d_out, void* d_workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GRANDPLUS_INFER_CHAIN_H */
