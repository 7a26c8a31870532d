/*
 * grandplus_step.h -- the device-resident state of a training step and the entry points that read it (implemented by
 * grand_plus_amd/csrc/step_state.hip and, for gp_clip_adam_step_dev, grand_plus_amd/csrc/optim.hip).
 *
 * Part of the ABI that grandplus.h describes (GP_ABI_VERSION, the status codes, gp_optim_tensor and the GP_OPTIM_* flags
 * are defined there): grandplus.h includes this file, so callers include grandplus.h alone.  The ctypes binding declares
 * the entry points under this file's name in _native.ABI and mirrors the two structs, and tests/test_host_abi.py holds
 * both against this file type by type.
 */
#ifndef GRANDPLUS_STEP_H
#define GRANDPLUS_STEP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Four inputs of a GRAND+ training step used to be host numbers: the DropNode seed, the MLP's dropout seed, the
 * consistency weight min(lam, lam * num_batch / warmup) (model.py:329) and Adam's step count.  A captured step would
 * freeze them.  Here they live in one small struct in DEVICE memory that the step itself advances, so the
 * whole step is a fixed sequence of launches with fixed arguments.
 *
 * gp_step_state: 88 bytes, 8-byte aligned, the caller's (zeroed before the first gp_step_advance).
 *   tick       the number of steps begun (Adam's step count of the current step)
 *   seed       the seed of the current step: mix(base_seed ^ tick * GP_STEP_MUL), mix of grandplus.h's gp_sample_seed
 *              (grand_plus_amd._common.step_seed mirrors it); both random_prop_rows and the MLP take it
 *   weight     the consistency weight of the current step: (float)min(lam, lam * (tick - 1) / warmup), formed in double
 *   step_size  per parameter group g < n_groups: (float)(lr[g] / (1 - beta1[g]^tick)), formed in double
 *   rsqrt_bc2  per parameter group: (float)(1 / sqrt(1 - beta2[g]^tick)), formed in double
 * ------------------------------------------------------------------------------------------ */
#define GP_STEP_MAX_GROUPS 8
#define GP_STEP_MAX_LAYERS 8
#define GP_STEP_MUL 0x8CB92BA72F3D8DD7ull

typedef struct gp_step_state {
    uint64_t tick;
    uint64_t seed;
    float weight;
    float step_size[GP_STEP_MAX_GROUPS];
    float rsqrt_bc2[GP_STEP_MAX_GROUPS];
} gp_step_state;

/* One launch of one thread: tick += 1, then seed, weight and the n_groups bias corrections of the new tick, in that
 * order, with plain stores.  lr / beta1 / beta2 are HOST arrays of n_groups doubles; they and every other argument travel
 * by value in the kernel arguments, so nothing is uploaded.  -ffp-contract=off as everywhere.
 * Checked before the device is touched: GP_ERR_NULL for d_state (or an array with n_groups > 0) missing;
 * GP_ERR_INVALID_ARG for n_groups outside [0, GP_STEP_MAX_GROUPS], lam not finite, warmup not finite or <= 0, an lr not
 * finite or a beta outside [0, 1).  Nothing on the call path synchronises, copies or allocates. */
int gp_step_advance(int device, gp_step_state* d_state, uint64_t base_seed, double lam, double warmup, int32_t n_groups,
                    const double* lr, const double* beta1, const double* beta2, void* stream);

/* ------------------------------------------------------------------------------------------
 * Every dropout mask of the current step as the explicit uint8 keep masks that the existing kernels take, from the seed
 * in d_state: one grid-stride launch over all segments, every offset a size_t.
 *
 *   GP_STEP_SEG_ROWS   the DropNode mask of gp_random_prop_rows_multi (d_keep, keep_stride = S_rows * K there):
 *                      for b < n_batch, k < min(d_filled[r], K), s < n_samples, r = d_batch_rows[b], e = r * K + k:
 *                          keep[s * keep_stride + e] = keep_scale(gp_sample_seed(seed, s), e, p) != 0
 *                      Only the batch's filled slots are written (a slot at or past keep_stride, or of a negative row, is
 *                      skipped); a repeated batch row writes the same bytes twice.  `width` and `layer` are not read.
 *   GP_STEP_SEG_LAYER  the mask of gp_mlp_block_forward's layer `layer` (d_keep [n_samples x n_batch x width] there):
 *                      for i < n_samples * n_batch * width, s = i / (n_batch * width), e = i % (n_batch * width):
 *                          keep[i] = keep_scale(GP_MLP_LAYER_SEED(gp_sample_seed(seed, s), layer), e, p) != 0
 *                      keep_stride, d_batch_rows, d_filled and K are not read.
 *
 * keep_scale is the counter hash of grandplus.h (u >= p keeps).  A segment with p == 0 is skipped and draws nothing, as
 * the kernels draw nothing there; p == 1 writes zeros.  `segments` is a HOST array of n_segments entries of DEVICE
 * pointers; it is copied into the kernel arguments.  n_segments == 0, or no segment with work, is GP_OK with nothing
 * launched.  Checked before the device is touched: GP_ERR_NULL for d_state, segments, a keep pointer or a rows segment's
 * d_batch_rows missing (d_filled NULL = every row holds K slots); GP_ERR_INVALID_ARG for n_segments outside
 * [0, 1 + GP_STEP_MAX_LAYERS], an unknown kind, n_samples outside [1, 16], n_batch < 0, p outside [0, 1], and for a
 * rows segment K outside [1, GP_MAX_K] or keep_stride < 0, for a layer segment width < 1 or layer outside
 * [0, GP_STEP_MAX_LAYERS).  No atomics; nothing on the call path synchronises, copies or allocates.
 * ------------------------------------------------------------------------------------------ */
#define GP_STEP_SEG_ROWS 0
#define GP_STEP_SEG_LAYER 1

typedef struct gp_step_segment {
    uint8_t* keep;
    int64_t keep_stride;
    const int32_t* batch_rows;
    const int32_t* filled;
    int32_t kind;
    int32_t n_samples;
    int32_t n_batch;
    int32_t K;
    int32_t width;
    int32_t layer;
    float p;
    int32_t pad;
} gp_step_segment;

int gp_step_masks(int device, const gp_step_state* d_state, const gp_step_segment* segments, int32_t n_segments, void* stream);

/* gp_clip_adam_step (grandplus.h) with step_size and rsqrt_bc2 read by the update kernel from two DEVICE floats -- a
 * group's entries of gp_step_state -- instead of taken by value: the same two kernels (the update kernel is one template,
 * instantiated on where the two numbers come from), the same arithmetic, flags, launch counts and contracts.  The two
 * pointers are required unless GP_OPTIM_NORM_ONLY is set (GP_ERR_NULL). */
int gp_clip_adam_step_dev(int device, const gp_optim_tensor* tensors, int32_t n_tensors, int flags,
                          float max_norm, float lr, double beta1, double beta2, float eps, float weight_decay,
                          const float* d_step_size, const float* d_rsqrt_bc2, void* d_workspace, float* d_norm_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GRANDPLUS_STEP_H */
