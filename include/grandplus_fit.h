/*
 * grandplus_fit.h -- the entry points of the sync-free fit loop (implemented by grand_plus_amd/csrc/fit.hip).
 *
 * Part of the ABI that grandplus.h describes (GP_ABI_VERSION and the status codes are defined there, gp_step_state in
 * grandplus_step.h): grandplus.h includes this file after grandplus_step.h, so callers include grandplus.h alone.  The
 * ctypes binding declares the entry points under this file's name in _native.ABI and mirrors the two structs, and
 * tests/test_host_abi.py holds both against this file type by type.
 *
 * Common contract: arguments are checked before the device is touched; no atomics; nothing on a call path allocates,
 * copies or synchronises; every argument travels by value in the kernel arguments, so each launch can be captured.
 */
#ifndef GRANDPLUS_FIT_H
#define GRANDPLUS_FIT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * The selection of the step the state is at, written into d_sel (int64 [n_labeled + u], u = min(unlabel_batch,
 * n_unlabel)): indices into the two pools, labelled first, the unlabelled ones offset by n_train -- what TrainStep
 * gathers rows and labels with.  One launch.  With t = d_state->tick (>= 1, read on the device),
 * nb = ceil(n_train / batch_size), epoch = (t - 1) / nb, lo = ((t - 1) % nb) * batch_size, perm of fit_perm.hpp and mix
 * the mix of gp_sample_seed:
 *     d_sel[i]             = perm(mix(base_seed ^ (epoch + 1) * GP_FIT_EPOCH_MUL), n_train, (lo + i) % n_train),  i < n_labeled
 *     d_sel[n_labeled + i] = n_train + perm(mix(d_state->seed ^ GP_FIT_UNLABEL_MUL), n_unlabel, i),               i < u
 * The labelled batches of an epoch are consecutive slices of one permutation, the last one short; the unlabelled batch is
 * the head of a fresh permutation every step.  n_labeled is the host's (a value of a capture): where it differs from
 * min(batch_size, n_train - lo), one thread sets bit 0 of *d_flag (never cleared here); the indices written are inside
 * their pools all the same.
 * GP_ERR_NULL: d_state, d_sel or d_flag missing.  GP_ERR_INVALID_ARG: n_train, n_unlabel, batch_size, unlabel_batch or
 * n_labeled outside [1, 2^31).
 * ------------------------------------------------------------------------------------------ */
int gp_fit_select(int device, const gp_step_state* d_state, uint64_t base_seed, int64_t n_train, int64_t n_unlabel,
                  int64_t batch_size, int64_t unlabel_batch, int64_t n_labeled, int64_t* d_sel, int32_t* d_flag, void* stream);

/* ------------------------------------------------------------------------------------------
 * gp_fit_track: the early-stop rule's state (model.py:297-300, 344-355), 40 bytes of DEVICE memory.  The caller writes
 * the initial image: best_loss = +inf, everything else 0.
 * ------------------------------------------------------------------------------------------ */
#define GP_FIT_STOP_ACC 0
#define GP_FIT_STOP_BOTH 1
#define GP_FIT_MAX_COPIES 32

typedef struct gp_fit_track {
    float best_loss;
    float best_acc;
    uint64_t best_tick;
    uint64_t stop_tick;
    int32_t bad_counter;
    int32_t n_evals;
    int32_t copy_now;
    int32_t stopped;
} gp_fit_track;

/* One thread applies the reference's rule to d_val = {loss, acc} (float32, as `valid` returns them), tick = d_state->tick:
 *     if stopped: copy_now = 0; return
 *     n_evals += 1; copy_now = 0
 *     if acc >= best_acc:
 *         if stop_mode == ACC or (stop_mode == BOTH and loss <= best_loss):
 *             best_loss, best_acc = loss, acc; best_tick = tick; bad_counter = 0; copy_now = 1
 *     else: bad_counter += 1
 *     if bad_counter >= patience: stopped = 1; stop_tick = tick
 * A NaN fails both comparisons.  Once stopped is set nothing changes again.
 * GP_ERR_NULL: d_track, d_val or d_state missing.  GP_ERR_INVALID_ARG: an unknown stop_mode, patience < 1. */
int gp_fit_track_update(int device, gp_fit_track* d_track, const float* d_val, const gp_step_state* d_state, int32_t stop_mode,
                        int32_t patience, void* stream);

/* src -> dst, n_words words of 4 bytes: DEVICE pointers, 4-byte aligned, not overlapping */
typedef struct gp_fit_copy {
    const void* src;
    void* dst;
    int64_t n_words;
} gp_fit_copy;

/* Copies every pair of the table when d_track->copy_now != 0 and does nothing otherwise: grid-stride launches of at most
 * GP_FIT_MAX_COPIES entries each (n_copies entries take ceil(n_copies / 32) launches; a group without words takes none).
 * `copies` is a HOST array; it is copied into the kernel arguments.  The decision is gp_fit_track_update's, an earlier
 * launch: every workgroup of the copy reads a decision made before the copy started.
 * GP_ERR_NULL: d_track, `copies` with n_copies > 0, or a pointer of an entry with words missing.  GP_ERR_INVALID_ARG:
 * n_copies < 0, n_words < 0, a pointer that is not 4-byte aligned. */
int gp_fit_snapshot(int device, const gp_fit_track* d_track, const gp_fit_copy* copies, int32_t n_copies, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GRANDPLUS_FIT_H */
