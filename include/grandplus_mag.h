/*
 * grandplus_mag.h -- MAG's fused front end of the C ABI: resident GFPush rows -> S augmented embeddings, forward and
 * backward (implemented by grand_plus_amd/csrc/mag_prop.hip).
 *
 * Part of the ABI that grandplus.h describes (GP_ABI_VERSION, GP_MAX_K and the status codes are defined there):
 * grandplus.h includes this file, so callers include grandplus.h alone.  The ctypes binding declares these entry points
 * under this file's name in _native.ABI, and tests/test_host_abi.py holds that table against this file type by type.
 */
#ifndef GRANDPLUS_MAG_H
#define GRANDPLUS_MAG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * One op for `MLP.emb` of every neighbour of a batch followed by `random_prop` (model_mag.py:48-55, 80-86, 354-356).
 * Batch row b names the resident row r = d_batch_rows[b] (NULL: r = b); its slot k < min(d_filled[r], K)
 * (d_filled NULL: K) holds node n = d_col[r*K + k], whose bag is the entries t = 0 .. len-1 of the node-attribute CSR
 * (id a_t = d_attr_indices[d_attr_indptr[n] + t], weight d_t = d_attr_data[...]):
 *
 *   e_{s,k}[h] = (sum_t (W[a_t,h] * m_in(s, r*K+k, t, h)) * d_t) * inv_den_n,   inv_den_n = 1 / (sum_t d_t + 1e-10)
 *   out[s,b,h] = (sum_k w'_{s,k} * e_{s,k}[h]) * inv_{s,b},                     inv_{s,b}  = 1 / (sum_k w'_{s,k} + 1e-12)
 *   w'_{s,k}   = (float)d_val[r*K+k] * m_node(s, r*K+k)
 *
 * DropNode, m_node: exactly gp_random_prop_rows_multi's mask, so one seed gives both ops the same DropNode decisions:
 *   hashed   keep_scale(gp_sample_seed(seed, s), r*K + k, dropnode_rate, 1 / (1 - dropnode_rate))
 *   explicit d_keep[s * keep_stride + r*K + k] ? 1 / (1 - dropnode_rate) : 0
 * (r is the resident row, not the batch position).
 * Input dropout, m_in: drawn per sample, per slot occurrence and per element, as the reference draws it on the gathered
 * [nnz, H] rows:
 *   GP_MAG_SLOT_SEED(seed, s, e) = mix(gp_sample_seed(seed, s) ^ ((e + 1) * 0xE7037ED1A0B428DB)),   e = r*K + k
 *   m_in(s, e, t, h) = keep_scale(GP_MAG_SLOT_SEED(seed, s, e), t * dim + h, input_droprate, 1 / (1 - input_droprate))
 * with mix, gp_sample_seed and keep_scale of the S-sample random_prop (grandplus.h); grand_plus_amd._common.mag_slot_seed
 * mirrors it.  With input_droprate == 0 or training == 0 nothing is drawn and e is computed once per slot and shared
 * by all samples.  training == 0 applies neither mask; a rate of 1 gives zeros; a rate of 0 draws nothing.
 *
 * Order contract (fp32, no contraction).  The workgroup of a batch row has n_waves = min(16, the power of two >= K)
 * waves: the map from slots to waves depends on K alone.
 *   - a bag is summed with t ascending, from 0.0f; its denominator sequentially in t;
 *   - wave w sums w' * e over its slots k = w, w + n_waves, ..., k ascending, from 0.0f;
 *   - the waves' sums are added with w ascending, from 0.0f; inv_{s,b}'s denominator is summed sequentially in k.
 * A slot whose weight is 0 in every sample of its chunk is skipped (its bag is never read); elsewhere it adds 0 * e.
 * Hence out[s] of an S-sample call equals the n_samples = 1 call with gp_sample_seed(seed, s) (or d_keep row s) bit for
 * bit, and the forward is bitwise equal run to run.  The backward recomputes both denominators in the forward's order;
 * it adds into d_dW with fp32 atomics, so it is NOT bitwise reproducible run to run.  Per slot it forms
 *   c_s[h] = (g[s,b,h] * inv_{s,b}) * w'_{s,k}
 * and adds, once per (entry t, h) and sample chunk, ((c[h] * inv_den_n) * d_t) with c = sum_s c_s, s ascending from
 * 0.0f (input dropout: sum_s ((c_s[h] * inv_den_n) * d_t) * m_in(s, e, t, h)); a value of exactly 0 is not added.
 *
 * Bounds: nothing out of range is ever used as an address.  A batch row outside [0, n_rows) gives a zero output row; a
 * slot whose column lies outside [0, n_nodes) is treated as absent (weight 0); an attribute id outside [0, n_vocab)
 * adds nothing to the numerator (its d_t stays in the bag's denominator, as for gp_embedding_bag).  Each is counted
 * once per occurrence into d_n_bad (NULL: not counted; caller-zeroed; ids are counted in the bags that are read), by
 * the forward only.
 *
 * Contracts: arguments are checked before the device is touched (GP_ERR_INVALID_ARG for n_samples outside [1, 16], K
 * outside [1, 1024], dim < 1, a negative size, a rate outside [0, 1], keep_stride < 1 with a mask; GP_ERR_NULL for a
 * missing pointer); n_batch == 0 returns GP_OK without a launch; one launch each, enqueued on `stream`; nothing on the
 * call path allocates, copies or synchronises.  d_out is [n_samples x n_batch x dim]; d_dW [n_vocab x dim] is zeroed
 * by the caller and added into.
 * ------------------------------------------------------------------------------------------ */
int gp_mag_prop_rows(int device, const float* d_weight, int64_t n_vocab, int32_t dim, const int64_t* d_attr_indptr,
                     const int32_t* d_attr_indices, const float* d_attr_data, int64_t n_nodes, const int32_t* d_col,
                     const double* d_val, const int32_t* d_filled, int64_t n_rows, int32_t K,
                     const int32_t* d_batch_rows, int32_t n_batch, int32_t n_samples, float dropnode_rate,
                     float input_droprate, int training, uint64_t seed, const uint8_t* d_keep, int64_t keep_stride,
                     float* d_out, int32_t* d_n_bad, void* stream);
int gp_mag_prop_rows_backward(int device, const float* d_grad_out, int64_t n_vocab, int32_t dim,
                              const int64_t* d_attr_indptr, const int32_t* d_attr_indices, const float* d_attr_data,
                              int64_t n_nodes, const int32_t* d_col, const double* d_val, const int32_t* d_filled,
                              int64_t n_rows, int32_t K, const int32_t* d_batch_rows, int32_t n_batch,
                              int32_t n_samples, float dropnode_rate, float input_droprate, int training,
                              uint64_t seed, const uint8_t* d_keep, int64_t keep_stride, float* d_dW, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GRANDPLUS_MAG_H */
