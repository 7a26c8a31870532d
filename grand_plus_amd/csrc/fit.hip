// fit.hip -- what the fit loop adds to a training step on the device (grandplus_fit.h):
//   fit_select_kernel    the step's selection into the two pools, from the tick and the seed in the step state: one thread
//                        per index, each a random access into a keyed permutation (fit_perm.hpp), so a replay needs no host input;
//   fit_track_kernel     one thread: the reference's early-stop rule (model.py:344-355) on the two floats of `valid`;
//   fit_snapshot_kernel  grid-stride copy of the model's tensors into their snapshot when the rule said so.
// The decision and the copy are two launches on purpose: every workgroup of the copy reads a decision made before the copy
// started.  The permutation is fit_perm.hpp's and the mixer gp_common.hpp's, called, not restated.  Plain C++ stores only;
// no atomics.
#include "gp_common.hpp"

#include "fit_perm.hpp"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxGrid = 4096;
constexpr long long kMaxSize = 1ll << 31;        // sizes are in [1, 2^31)

struct DeviceMix {
    __device__ __forceinline__ u64 operator()(u64 x) const { return mix64(x); }
};

struct SelectArgs {
    u64 base_seed;
    u32 n_train, n_unlabel, batch_size, n_labeled, u;
};

__global__ __launch_bounds__(kBlock) void fit_select_kernel(const gp_step_state* __restrict__ st, const SelectArgs a,
                                                            long long* __restrict__ sel, int* __restrict__ flag)
{
    const gp_fit::StepSlice sl = gp_fit::step_slice(st->tick, a.n_train, a.batch_size);
    const u64 labelled_key = gp_fit::epoch_key(DeviceMix(), a.base_seed, sl.epoch);
    const u64 unlabelled_key = gp_fit::unlabel_key(DeviceMix(), st->seed);
    const size_t total = (size_t)a.n_labeled + a.u;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock) {
        if (i < a.n_labeled) {
            const u32 at = (u32)(((u64)sl.lo + i) % a.n_train);                  // inside the pool whatever n_labeled is
            sel[i] = (long long)gp_fit::perm(DeviceMix(), labelled_key, a.n_train, at);
        } else {
            sel[i] = (long long)a.n_train + (long long)gp_fit::perm(DeviceMix(), unlabelled_key, a.n_unlabel, (u32)(i - a.n_labeled));
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && sl.n_labeled != a.n_labeled) *flag = *flag | 1;   // the host picked the wrong shape
}

__global__ void fit_track_kernel(gp_fit_track* __restrict__ tr, const float* __restrict__ val, const gp_step_state* __restrict__ st,
                                 const int mode, const int patience)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    if (tr->stopped) { tr->copy_now = 0; return; }
    const float loss = val[0], acc = val[1];
    const u64 tick = st->tick;
    int bad = tr->bad_counter, copy = 0;
    tr->n_evals = tr->n_evals + 1;
    if (acc >= tr->best_acc) {
        if (mode == GP_FIT_STOP_ACC || loss <= tr->best_loss) {                  // the other mode is GP_FIT_STOP_BOTH
            tr->best_loss = loss;
            tr->best_acc = acc;
            tr->best_tick = tick;
            bad = 0;
            copy = 1;
        }                                                                        // else neither reset nor counted: the reference's gap
    } else {
        ++bad;
    }
    tr->bad_counter = bad;
    tr->copy_now = copy;
    if (bad >= patience) { tr->stopped = 1; tr->stop_tick = tick; }
}

struct CopyEntry {
    const u32* src;
    u32* dst;
    size_t end;                    // words of this and every earlier entry of the table
};

struct CopyTable {
    CopyEntry e[GP_FIT_MAX_COPIES];
    int n;
};

static_assert(sizeof(CopyTable) <= 1024, "the table travels in the kernel arguments");

__global__ __launch_bounds__(kBlock) void fit_snapshot_kernel(const gp_fit_track* __restrict__ tr, const CopyTable tab)
{
    if (tr->copy_now == 0) return;
    const size_t total = tab.e[tab.n - 1].end;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock) {
        int lo = 0, hi = tab.n - 1;                                   // the first entry whose end exceeds i
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (i < tab.e[mid].end) hi = mid; else lo = mid + 1;
        }
        const size_t j = i - (lo > 0 ? tab.e[lo - 1].end : 0);
        tab.e[lo].dst[j] = tab.e[lo].src[j];
    }
}

}  // namespace

extern "C" {

int gp_fit_select(int device, const gp_step_state* d_state, uint64_t base_seed, int64_t n_train, int64_t n_unlabel,
                  int64_t batch_size, int64_t unlabel_batch, int64_t n_labeled, int64_t* d_sel, int32_t* d_flag, void* stream)
{
    const char* where = "gp_fit_select";
    for (const int64_t v : {n_train, n_unlabel, batch_size, unlabel_batch, n_labeled})
        if (v < 1 || v >= kMaxSize)
            return fail(GP_ERR_INVALID_ARG, where, "n_train, n_unlabel, batch_size, unlabel_batch or n_labeled is outside [1, 2^31)");
    if (!d_state || !d_sel || !d_flag) return fail(GP_ERR_NULL, where, "the state, the selection or the flag is NULL");
    const SelectArgs a = {base_seed, (u32)n_train, (u32)n_unlabel, (u32)batch_size, (u32)n_labeled,
                          (u32)(unlabel_batch < n_unlabel ? unlabel_batch : n_unlabel)};
    if (const int rc = set_device(device, where)) return rc;
    const size_t blocks = ((size_t)a.n_labeled + a.u + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(fit_select_kernel, dim3((unsigned)(blocks < (size_t)kMaxGrid ? blocks : (size_t)kMaxGrid)), dim3(kBlock), 0,
                       (hipStream_t)stream, d_state, a, (long long*)d_sel, (int*)d_flag);
    return launch_status("fit_select_kernel");
}

int gp_fit_track_update(int device, gp_fit_track* d_track, const float* d_val, const gp_step_state* d_state, int32_t stop_mode,
                        int32_t patience, void* stream)
{
    const char* where = "gp_fit_track_update";
    if ((stop_mode != GP_FIT_STOP_ACC && stop_mode != GP_FIT_STOP_BOTH) || patience < 1)
        return fail(GP_ERR_INVALID_ARG, where, "stop_mode is unknown or patience < 1");
    if (!d_track || !d_val || !d_state) return fail(GP_ERR_NULL, where, "the track, the validation result or the state is NULL");
    if (const int rc = set_device(device, where)) return rc;
    hipLaunchKernelGGL(fit_track_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, d_track, d_val, d_state, (int)stop_mode, (int)patience);
    return launch_status("fit_track_kernel");
}

int gp_fit_snapshot(int device, const gp_fit_track* d_track, const gp_fit_copy* copies, int32_t n_copies, void* stream)
{
    const char* where = "gp_fit_snapshot";
    if (n_copies < 0) return fail(GP_ERR_INVALID_ARG, where, "n_copies < 0");
    if (!d_track || (n_copies > 0 && !copies)) return fail(GP_ERR_NULL, where, "the track or the copy table is NULL");
    for (int i = 0; i < n_copies; ++i) {
        const gp_fit_copy& c = copies[i];
        if (c.n_words < 0 || ((uintptr_t)c.src & 3) || ((uintptr_t)c.dst & 3))
            return fail(GP_ERR_INVALID_ARG, where, "an entry has n_words < 0 or a pointer that is not 4-byte aligned");
        if (c.n_words > 0 && (!c.src || !c.dst)) return fail(GP_ERR_NULL, where, "an entry's src or dst is NULL");
    }
    bool device_set = false;
    for (int first = 0; first < n_copies; first += GP_FIT_MAX_COPIES) {
        CopyTable tab = {};
        size_t total = 0;
        for (int i = first; i < n_copies && i < first + GP_FIT_MAX_COPIES; ++i) {
            if (copies[i].n_words == 0) continue;
            total += (size_t)copies[i].n_words;
            tab.e[tab.n++] = {(const u32*)copies[i].src, (u32*)copies[i].dst, total};
        }
        if (total == 0) continue;
        if (!device_set) {
            if (const int rc = set_device(device, where)) return rc;
            device_set = true;
        }
        const size_t blocks = (total + kBlock - 1) / kBlock;
        hipLaunchKernelGGL(fit_snapshot_kernel, dim3((unsigned)(blocks < (size_t)kMaxGrid ? blocks : (size_t)kMaxGrid)), dim3(kBlock), 0,
                           (hipStream_t)stream, d_track, tab);
        if (const int rc = launch_status("fit_snapshot_kernel")) return rc;
    }
    return GP_OK;
}

}  // extern "C"
