// optim_defer.hip -- DESIGN §7za: the exact (dense) Adam trajectory of MAG's embedding table at the memory traffic of the
// touched rows.
//
// Under dense Adam (model_mag.py:312) a row no batch touches still moves while its moments decay: at step t it takes
// adam_element(p, 0.0f, m, v, coef_t, a_t), a recurrence over the element's own (p, m, v) and three numbers of the step.
// Nobody reads the row while it is untouched, so the update is put off: the three numbers of every step stand in a ring,
// last[r] says which step row r is current through, and the missed steps are replayed in order, through the same
// adam_element, just before the row is next read (the pre-forward catch-up of the batch's rows) and whenever the outside
// world looks at the table (the flush).  Same function, same order, nothing fused: the bits are the dense path's.
//   optim_defer_catch_up_kernel   a wave per list position; the heads' rows through T - 1;
//   optim_defer_step_kernel       optim_rows_adam_kernel<lazy>'s windows; workgroup 0 writes the ring entry of step T; a
//                                 head row is brought through T - 1 (normally no trip), stepped, and last[r] = T;
//   optim_defer_flush_kernel      a wave per 64 rows, capped grid: every row through T.
// The served gap, the ring's slots and tags and what an unserved row keeps are optim_defer_layout.hpp's (HIP-free, held
// on the CPU by tests/native/optim_defer_check.cpp); heads are optim_rows_layout.hpp's; the element update and the clip
// coefficient are optim_math.hpp's.  No kernel writes a counter that other workgroups of its launch read: T is the step
// state's tick, advanced once per step by gp_step_advance.  Plain C++ stores, no atomics, no host read.
#include "optim_math.hpp"
#include "optim_rows_layout.hpp"
#include "optim_rows_heads.hpp"
#include "optim_defer_layout.hpp"
#include "optim_defer_abi.hpp"

namespace {

using gp_optim_defer::Entry;

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kSlots = GP_OPTIM_WORKSPACE_BYTES / 8;           // optim.hip's f64 partials of the squared norm
constexpr int kStepGrid = kSlots;                              // the step's windows: optim_rows.hip's cap
constexpr int kCatchGrid = 8192;                               // workgroups of the catch-up: kWaves list positions each per trip
constexpr int kFlushGrid = 2048;                               // workgroups of the flush: kWaves * 64 rows each per trip
constexpr int kRowsAtOnce = 8;                                 // head rows whose loads are in flight together (optim_rows.hip's)

static_assert(kSlots == kBlock * 4, "clip_coef reads four slots per thread");

struct DeferArgs {
    float* p; float* m; float* v;
    int* last;
    const Entry* hist;
    int* flag;
    const u64* tick;
    long long V;
    int H, capacity;
};

// lane j's x in every lane (j wave-uniform): the entry of a step goes from the lane that loaded it to all, without a load
__device__ __forceinline__ float lane_value(float x, int j)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), j));
}

// Replays the steps last[row] + 1 .. through on one row: a wave per row, lanes over H, so the trip count is wave-uniform.
// To be called by a whole wave.  The ring is read 64 steps at a time, lane j the entry of step s0 + j: one load per 64 steps
// off the replay's chain of dependent updates.  Returns false, with the flag bit set and nothing written, when the row cannot
// be served.
__device__ __forceinline__ bool catch_up_row(const DeferArgs& D, const AdamArgs& a, long long row, u64 tick, long long through, int lane)
{
    const long long last = __builtin_amdgcn_readfirstlane(D.last[row]);
    const gp_optim_defer::Plan what = gp_optim_defer::plan(tick, last, through, D.capacity);
    if (what == gp_optim_defer::kNothing) return true;
    bool served = what == gp_optim_defer::kReplay;
    for (long long s0 = last + 1; served && s0 <= through; s0 += 64) {             // every tag, before the first element is touched
        const long long mine = s0 + lane;
        served = !__ballot(mine <= through && !gp_optim_defer::tag_ok(D.hist[gp_optim_defer::slot(mine, D.capacity)], mine));
    }
    if (!served) {
        if (lane == 0) *D.flag = *D.flag | gp_optim_defer::kFlagBit;                 // a plain store; every writer sets the same bit
        return false;
    }
    for (long long s0 = last + 1; s0 <= through; s0 += 64) {                       // wave-uniform
        const long long mine = s0 + lane;
        Entry e = {};
        if (mine <= through) e = D.hist[gp_optim_defer::slot(mine, D.capacity)];
        const int n = through - s0 + 1 < 64 ? (int)(through - s0 + 1) : 64;
        for (int h = lane; h < D.H; h += 64) {
            const long long at = row * D.H + h;
            float p = D.p[at], m = D.m[at], v = D.v[at];
            for (int j = 0; j < n; ++j) {
                AdamArgs b = a;
                b.step_size = lane_value(e.step_size, j);
                b.rsqrt_bc2 = lane_value(e.rsqrt_bc2, j);
                adam_element(p, 0.0f, m, v, lane_value(e.coef, j), b);
            }
            D.p[at] = p; D.m[at] = m; D.v[at] = v;
        }
    }
    if (lane == 0) D.last[row] = (int)through;
    return true;
}

__global__ __launch_bounds__(kBlock) void optim_defer_catch_up_kernel(const DeferArgs D, const AdamArgs a,
                                                                       const long long* __restrict__ keys, long long n_sorted)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 tick = *D.tick;
    if (tick == 0) return;                                                         // no step has begun: nothing lags
    for (long long i = (long long)blockIdx.x * kWaves + wave; i < n_sorted; i += (long long)gridDim.x * kWaves) {   // wave-uniform
        if (!gp_optim_rows::is_head(keys, i, D.V)) continue;
        catch_up_row(D, a, keys[i], tick, (long long)tick - 1, lane);
    }
}

__global__ __launch_bounds__(kBlock) void optim_defer_flush_kernel(const DeferArgs D, const AdamArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 tick = *D.tick;
    const long long n_win = (D.V + 63) >> 6;
    for (long long win = (long long)blockIdx.x * kWaves + wave; win < n_win; win += (long long)gridDim.x * kWaves) {   // wave-uniform
        const long long row = (win << 6) + lane;
        // a row that is current costs this read; anything else, the unservable included, goes through catch_up_row
        u64 todo = __ballot(row < D.V && (u64)(long long)D.last[row] != tick);
        while (todo) {
            const int l = __builtin_ctzll(todo);
            todo &= todo - 1;
            catch_up_row(D, a, (win << 6) + l, tick, (long long)tick, lane);
        }
    }
}

__global__ __launch_bounds__(kBlock) void optim_defer_step_kernel(const DeferArgs D, Entry* hist_out,
                                                                   const float* __restrict__ dW, const long long* __restrict__ keys,
                                                                   long long n_sorted, const double* __restrict__ partials,
                                                                   float* __restrict__ norm_out, const AdamArgs a_in,
                                                                   const float* __restrict__ d_step_size,
                                                                   const float* __restrict__ d_rsqrt_bc2)
{
    __shared__ double lds[kWaves];
    AdamArgs a = a_in;
    a.step_size = *d_step_size;
    a.rsqrt_bc2 = *d_rsqrt_bc2;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float norm;
    const float coef = clip_coef<kWaves>(partials, a.max_norm, lds, norm);
    const u64 tick = *D.tick;
    const long long T = (long long)tick;
    if (blockIdx.x == 0 && tid == 0) {
        *norm_out = norm;
        // the entry of step T; no workgroup of this launch reads its slot (the oldest step replayed here is T - capacity + 1)
        Entry e;
        e.step_size = a.step_size; e.rsqrt_bc2 = a.rsqrt_bc2; e.coef = coef; e.tag = gp_optim_defer::tag(T);
        hist_out[gp_optim_defer::slot(T, D.capacity)] = e;
    }
    const int H = D.H;
    const long long n_win = gp_optim_rows::windows(n_sorted);
    for (long long win = (long long)blockIdx.x * kWaves + wave; win < n_win; win += (long long)gridDim.x * kWaves) {   // wave-uniform
        const long long i = (win << 6) + lane;
        const bool in = i < n_sorted;
        const long long key = in ? keys[i] : D.V;
        u64 heads = __ballot(in && gp_optim_rows::is_head(keys, i, D.V));
        while (heads) {
            long long rows[kRowsAtOnce];
            const int n = take_heads(heads, key, rows);
            bool current = tick <= (u64)INT32_MAX;                                 // every row of the group is through T - 1
#pragma unroll
            for (int r = 0; r < kRowsAtOnce; ++r)
                if (r < n) current = current && (long long)D.last[rows[r]] == T - 1;
            if (current) {                                                         // the common case: optim_rows.hip's lazy update
                for (int h0 = 0; h0 < H; h0 += 64) {
                    const int h = h0 + lane;
                    if (h >= H) continue;
                    float g[kRowsAtOnce], p[kRowsAtOnce], m[kRowsAtOnce], v[kRowsAtOnce];
#pragma unroll
                    for (int r = 0; r < kRowsAtOnce; ++r) {
                        if (r < n) {
                            const long long at = rows[r] * H + h;
                            g[r] = dW[at]; p[r] = D.p[at]; m[r] = D.m[at]; v[r] = D.v[at];
                        }
                    }
#pragma unroll
                    for (int r = 0; r < kRowsAtOnce; ++r) {
                        if (r < n) {
                            const long long at = rows[r] * H + h;
                            adam_element(p[r], g[r], m[r], v[r], coef, a);
                            D.p[at] = p[r]; D.m[at] = m[r]; D.v[at] = v[r];
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < kRowsAtOnce; ++r)
                    if (r < n && lane == 0) D.last[rows[r]] = (int)T;
                continue;
            }
            for (int r = 0; r < n; ++r) {                                          // a row the pre-forward list missed: one at a time
                const long long row = rows[r];
                if (!catch_up_row(D, a, row, tick, T - 1, lane)) continue;         // unserved: not stepped either
                for (int h = lane; h < H; h += 64) {
                    const long long at = row * H + h;
                    float p = D.p[at], m = D.m[at], v = D.v[at];
                    adam_element(p, dW[at], m, v, coef, a);
                    D.p[at] = p; D.m[at] = m; D.v[at] = v;
                }
                if (lane == 0) D.last[row] = (int)T;
            }
        }
    }
}

int grid_for(long long units, int cap)
{
    const long long g = (units + kWaves - 1) / kWaves;
    return (int)(g < 1 ? 1 : g < cap ? g : cap);
}

// what every entry checks, before the device is touched
int defer_check(const char* where, int64_t n_vocab, int32_t dim, double beta1, double beta2, float eps, float weight_decay,
                int32_t capacity, const void* d_param, const void* d_exp_avg, const void* d_exp_avg_sq, const void* d_tick,
                const void* d_last, const void* d_hist, const void* d_flag)
{
    if (n_vocab < 1 || dim < 1) return fail(GP_ERR_INVALID_ARG, where, "n_vocab < 1 or dim < 1");
    if (n_vocab > INT64_MAX / dim) return fail(GP_ERR_INVALID_ARG, where, "n_vocab * dim does not fit 63 bits");
    if (!gp_optim_defer::valid_capacity(capacity)) return fail(GP_ERR_INVALID_ARG, where, "capacity is no power of two in [4, 65536]");
    if (!std::isfinite(beta1) || !std::isfinite(beta2) || !std::isfinite(eps) || !std::isfinite(weight_decay))
        return fail(GP_ERR_INVALID_ARG, where, "a hyper-parameter is not finite");
    if (!d_param || !d_exp_avg || !d_exp_avg_sq || !d_tick || !d_last || !d_hist || !d_flag)
        return fail(GP_ERR_NULL, where, "the table, its state, d_tick, d_last, d_hist or d_flag is NULL");
    return GP_OK;
}

AdamArgs adam_args(float max_norm, double beta1, double beta2, float eps, float weight_decay)
{
    return {max_norm, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, weight_decay, 0.0f, 0.0f, 0};
}

}  // namespace

extern "C" {

int gp_optim_defer_catch_up(int device, float* d_param, float* d_exp_avg, float* d_exp_avg_sq, const int64_t* d_keys,
                            int64_t n_sorted, int64_t n_vocab, int32_t dim, double beta1, double beta2, float eps,
                            float weight_decay, const uint64_t* d_tick, int32_t* d_last, const void* d_hist, int32_t capacity,
                            int32_t* d_flag, void* stream)
{
    const char* where = "gp_optim_defer_catch_up";
    if (n_sorted < 0) return fail(GP_ERR_INVALID_ARG, where, "n_sorted < 0");
    if (const int rc = defer_check(where, n_vocab, dim, beta1, beta2, eps, weight_decay, capacity, d_param, d_exp_avg, d_exp_avg_sq,
                                   d_tick, d_last, d_hist, d_flag)) return rc;
    if (!d_keys) return fail(GP_ERR_NULL, where, "d_keys is NULL");
    if (n_sorted == 0) return GP_OK;                                              // nothing is listed
    if (const int rc = set_device(device, where)) return rc;
    const DeferArgs D = {d_param, d_exp_avg, d_exp_avg_sq, d_last, static_cast<const Entry*>(d_hist), d_flag, (const u64*)d_tick,
                         (long long)n_vocab, dim, capacity};
    hipLaunchKernelGGL(optim_defer_catch_up_kernel, dim3(grid_for(n_sorted, kCatchGrid)), dim3(kBlock), 0, (hipStream_t)stream, D,
                       adam_args(0.0f, beta1, beta2, eps, weight_decay), (const long long*)d_keys, (long long)n_sorted);
    return launch_status("optim_defer_catch_up_kernel");
}

int gp_optim_defer_step(int device, float* d_param, float* d_exp_avg, float* d_exp_avg_sq, const float* d_dW,
                        const int64_t* d_keys, int64_t n_sorted, int64_t n_vocab, int32_t dim, float max_norm, float lr,
                        double beta1, double beta2, float eps, float weight_decay, const float* d_step_size,
                        const float* d_rsqrt_bc2, const uint64_t* d_tick, int32_t* d_last, void* d_hist, int32_t capacity,
                        int32_t* d_flag, void* d_workspace, float* d_norm_out, void* stream)
{
    const char* where = "gp_optim_defer_step";
    if (n_sorted < 0) return fail(GP_ERR_INVALID_ARG, where, "n_sorted < 0");
    if (!std::isfinite(max_norm) || !std::isfinite(lr)) return fail(GP_ERR_INVALID_ARG, where, "a hyper-parameter is not finite");
    if (const int rc = defer_check(where, n_vocab, dim, beta1, beta2, eps, weight_decay, capacity, d_param, d_exp_avg, d_exp_avg_sq,
                                   d_tick, d_last, d_hist, d_flag)) return rc;
    if (!d_dW || !d_keys || !d_step_size || !d_rsqrt_bc2 || !d_workspace || !d_norm_out)
        return fail(GP_ERR_NULL, where, "d_dW, d_keys, d_step_size, d_rsqrt_bc2, the workspace or the norm output is NULL");
    if (const int rc = set_device(device, where)) return rc;
    const DeferArgs D = {d_param, d_exp_avg, d_exp_avg_sq, d_last, static_cast<const Entry*>(d_hist), d_flag, (const u64*)d_tick,
                         (long long)n_vocab, dim, capacity};
    // at least workgroup 0, which writes the step's history: an empty batch is still a step
    hipLaunchKernelGGL(optim_defer_step_kernel, dim3(grid_for(gp_optim_rows::windows(n_sorted), kStepGrid)), dim3(kBlock), 0,
                       (hipStream_t)stream, D, static_cast<Entry*>(d_hist), d_dW, (const long long*)d_keys, (long long)n_sorted,
                       static_cast<const double*>(d_workspace), d_norm_out, adam_args(max_norm, beta1, beta2, eps, weight_decay),
                       d_step_size, d_rsqrt_bc2);
    return launch_status("optim_defer_step_kernel");
}

int gp_optim_defer_flush(int device, float* d_param, float* d_exp_avg, float* d_exp_avg_sq, int64_t n_vocab, int32_t dim,
                         double beta1, double beta2, float eps, float weight_decay, const uint64_t* d_tick, int32_t* d_last,
                         const void* d_hist, int32_t capacity, int32_t* d_flag, void* stream)
{
    const char* where = "gp_optim_defer_flush";
    if (const int rc = defer_check(where, n_vocab, dim, beta1, beta2, eps, weight_decay, capacity, d_param, d_exp_avg, d_exp_avg_sq,
                                   d_tick, d_last, d_hist, d_flag)) return rc;
    if (const int rc = set_device(device, where)) return rc;
    const DeferArgs D = {d_param, d_exp_avg, d_exp_avg_sq, d_last, static_cast<const Entry*>(d_hist), d_flag, (const u64*)d_tick,
                         (long long)n_vocab, dim, capacity};
    hipLaunchKernelGGL(optim_defer_flush_kernel, dim3(grid_for((n_vocab + 63) >> 6, kFlushGrid)), dim3(kBlock), 0, (hipStream_t)stream,
                       D, adam_args(0.0f, beta1, beta2, eps, weight_decay));
    return launch_status("optim_defer_flush_kernel");
}

}  // extern "C"
