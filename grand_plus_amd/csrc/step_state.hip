// step_state.hip -- the device-resident state of a GRAND+ training step (grandplus_step.h).
//
// A step's DropNode seed, dropout seed, consistency weight (model.py:329) and Adam step count used to be host numbers.
// Here they are one gp_step_state in device memory:
//   step_advance_kernel   one thread: ++tick, then the seed, the weight and every group's bias corrections of the new tick;
//   step_masks_kernel     every dropout mask of the step, from the seed in the state, as the uint8 keep masks that
//                         random_prop_rows and the MLP blocks already take: grid-stride over the items of all segments.
// No tuned kernel changes for this: the masks are what carries the device seed into them.  The hash and the seed
// derivations are gp_common.hpp's and dropnode.hpp's, called, not restated.  Plain C++ stores only; no atomics.
#include "dropnode.hpp"

#include <cmath>

namespace {

constexpr int kBlock = 256;
constexpr int kMaxGrid = 4096;
constexpr int kMaxSegments = 1 + GP_STEP_MAX_LAYERS;

struct AdvanceArgs {
    u64 base_seed;
    double lam, warmup;
    double lr[GP_STEP_MAX_GROUPS], beta1[GP_STEP_MAX_GROUPS], beta2[GP_STEP_MAX_GROUPS];
    int n_groups;
};

__global__ void step_advance_kernel(gp_step_state* __restrict__ st, const AdvanceArgs a)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const u64 t = st->tick + 1;
    st->tick = t;
    st->seed = mix64(a.base_seed ^ (t * GP_STEP_MUL));
    const double ramp = a.lam * (double)(t - 1) / a.warmup;              // num_batch of model.py:329 starts at 0
    st->weight = (float)(a.lam < ramp ? a.lam : ramp);
    for (int g = 0; g < a.n_groups; ++g) {
        st->step_size[g] = (float)(a.lr[g] / (1.0 - pow(a.beta1[g], (double)t)));
        st->rsqrt_bc2[g] = (float)(1.0 / sqrt(1.0 - pow(a.beta2[g], (double)t)));
    }
}

struct Segment {
    unsigned char* keep;
    size_t keep_stride;            // rows: S_rows * K
    const int* batch_rows;         // rows
    const int* filled;             // rows, or NULL
    size_t per_sample;             // rows: n_batch * K; layer: n_batch * width
    size_t end;                    // items of this and every earlier segment of the table
    int kind, n_samples, K, layer;
    float p;
};

struct SegmentTable {
    Segment s[kMaxSegments];
    int n;
};

static_assert(sizeof(SegmentTable) <= 1024, "the table travels in the kernel arguments");

__global__ __launch_bounds__(kBlock) void step_masks_kernel(const gp_step_state* __restrict__ st, const SegmentTable tab)
{
    const u64 seed = st->seed;
    const size_t total = tab.s[tab.n - 1].end;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock) {
        int g = 0;
        while (i >= tab.s[g].end) ++g;
        const Segment& sg = tab.s[g];
        const size_t j = i - (g > 0 ? tab.s[g - 1].end : 0);
        const int s = (int)(j / sg.per_sample);
        const size_t e = j % sg.per_sample;
        if (sg.kind == GP_STEP_SEG_LAYER) {
            sg.keep[j] = keep_scale(layer_sample_seed(seed, s, sg.layer), (u64)e, sg.p, inv_keep(sg.p)) != 0.0f;
        } else {
            const size_t b = e / (size_t)sg.K;
            const int k = (int)(e % (size_t)sg.K);
            const int r = sg.batch_rows[b];
            if (r < 0) continue;
            const size_t slot = (size_t)r * (size_t)sg.K + (size_t)k;
            if (slot >= sg.keep_stride || k >= row_len(sg.filled, r, sg.K)) continue;
            sg.keep[(size_t)s * sg.keep_stride + slot] = keep_scale(sample_seed(seed, s), (u64)slot, sg.p, inv_keep(sg.p)) != 0.0f;
        }
    }
}

}  // namespace

extern "C" {

int gp_step_advance(int device, gp_step_state* d_state, uint64_t base_seed, double lam, double warmup, int32_t n_groups,
                    const double* lr, const double* beta1, const double* beta2, void* stream)
{
    const char* where = "gp_step_advance";
    if (n_groups < 0 || n_groups > GP_STEP_MAX_GROUPS)
        return fail(GP_ERR_INVALID_ARG, where, "n_groups is outside [0, GP_STEP_MAX_GROUPS = 8]");
    if (!std::isfinite(lam) || !std::isfinite(warmup) || !(warmup > 0.0))
        return fail(GP_ERR_INVALID_ARG, where, "lam is not finite, or warmup is not finite and > 0");
    if (!d_state || (n_groups > 0 && (!lr || !beta1 || !beta2)))
        return fail(GP_ERR_NULL, where, "the state or a hyper-parameter array is NULL");
    AdvanceArgs a = {};
    a.base_seed = base_seed; a.lam = lam; a.warmup = warmup; a.n_groups = n_groups;
    for (int g = 0; g < n_groups; ++g) {
        if (!std::isfinite(lr[g]) || !(beta1[g] >= 0.0 && beta1[g] < 1.0) || !(beta2[g] >= 0.0 && beta2[g] < 1.0))
            return fail(GP_ERR_INVALID_ARG, where, "an lr is not finite or a beta is outside [0, 1)");
        a.lr[g] = lr[g]; a.beta1[g] = beta1[g]; a.beta2[g] = beta2[g];
    }
    if (const int rc = set_device(device, where)) return rc;
    hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, d_state, a);
    return launch_status("step_advance_kernel");
}

int gp_step_masks(int device, const gp_step_state* d_state, const gp_step_segment* segments, int32_t n_segments, void* stream)
{
    const char* where = "gp_step_masks";
    if (n_segments < 0 || n_segments > kMaxSegments)
        return fail(GP_ERR_INVALID_ARG, where, "n_segments is outside [0, 1 + GP_STEP_MAX_LAYERS = 9]");
    if (!d_state || (n_segments > 0 && !segments)) return fail(GP_ERR_NULL, where, "the state or the segment table is NULL");
    SegmentTable tab = {};
    size_t total = 0;
    for (int i = 0; i < n_segments; ++i) {
        const gp_step_segment& g = segments[i];
        const bool rows = g.kind == GP_STEP_SEG_ROWS;
        if (!rows && g.kind != GP_STEP_SEG_LAYER) return fail(GP_ERR_INVALID_ARG, where, "a segment's kind is unknown");
        if (g.n_samples < 1 || g.n_samples > kMaxSamples || g.n_batch < 0 || !(g.p >= 0.0f && g.p <= 1.0f))
            return fail(GP_ERR_INVALID_ARG, where, "a segment has n_samples outside [1, 16], n_batch < 0 or p outside [0, 1]");
        if (rows && (g.K < 1 || g.K > GP_MAX_K || g.keep_stride < 0))
            return fail(GP_ERR_INVALID_ARG, where, "a rows segment has K outside [1, GP_MAX_K] or keep_stride < 0");
        if (!rows && (g.width < 1 || g.layer < 0 || g.layer >= GP_STEP_MAX_LAYERS))
            return fail(GP_ERR_INVALID_ARG, where, "a layer segment has width < 1 or layer outside [0, GP_STEP_MAX_LAYERS)");
        if (!g.keep || (rows && !g.batch_rows)) return fail(GP_ERR_NULL, where, "a segment's keep or batch_rows is NULL");
        if (g.p == 0.0f || g.n_batch == 0) continue;                       // nothing is drawn, as in the kernels that read the mask
        const size_t per_sample = (size_t)g.n_batch * (size_t)(rows ? g.K : g.width);
        total += per_sample * (size_t)g.n_samples;
        tab.s[tab.n++] = {g.keep, (size_t)g.keep_stride, g.batch_rows, g.filled, per_sample, total, g.kind, g.n_samples,
                          g.K, g.layer, g.p};
    }
    if (total == 0) return GP_OK;
    if (const int rc = set_device(device, where)) return rc;
    const size_t blocks = (total + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(step_masks_kernel, dim3((unsigned)(blocks < (size_t)kMaxGrid ? blocks : (size_t)kMaxGrid)), dim3(kBlock), 0,
                       (hipStream_t)stream, d_state, tab);
    return launch_status("step_masks_kernel");
}

}  // extern "C"
