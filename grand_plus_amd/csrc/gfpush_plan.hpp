// gfpush_plan.hpp -- every host-side decision of a GFPush call, as functions of plain values.
//
// No HIP, no handle, no global state: this header includes the C++ standard library only and compiles with plain
// g++ -std=c++17, so tests/native/gfpush_plan_check.cpp runs every decision on a CPU, under the sanitizers.  gfpush.hip is the
// shell around it: it gathers the inputs (options, the running estimate, free memory, occupancy, CU count), calls the decision
// and applies it with HIP calls.  What the decisions need from the kernel headers comes in as one KernelConsts.
#pragma once

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

namespace gp {
namespace planning {

typedef unsigned long long cap_t;                // (the type of KParams' capacities)

enum Status { kOk = 0, kInvalidArg, kNoMem, kNeedOccupancy };

// The constants of gfpush_kernels.hpp / gfpush_sketch.hpp the decisions read (they depend on the build: GP_DIAG, GP_SK_TIMING,
// GP_FLAT_W, GP_MIN_CAP).  gfpush.hip fills one from them.
struct KernelConsts {
    int ctl_bytes = 0, three_lds = 0, min_cap = 0, topk_bins = 0, bucket_cap = 0, unit_shift = 0;
    int sk_max_pushers = 0, sk_max_coef = 0, sk_tie = 0;
};

// What gp_set_option writes on a single-GPU handle.
struct Options {
    int block_threads = 0; int lds_bytes = 0; int max_workgroups = 0;     // 0 = choose per graph
    int verify_merge = 0;                                                 // gp_gfpush re-checks every merged row against the slab once the launches have retired (option "verify_merge")
    int lds_pad = 0; int pretouch = 0;                                    // experiment knobs: extra dynamic LDS per workgroup that the tables do not use (forces fewer workgroups per CU); memset the workspace when it is allocated
    int64_t workspace_mb = 65536; int force_global = 0; int exact_stats = 0; int diag_flags = 0; int direct_tables = 1; int seedrow = 1; int solo_levels = 1;
    int kernel = 0;                                                        // option: 0 = choose per call, 1 = general kernel, 2 = sketch kernel whenever the call allows it
    int sk_block = 0, sk_lg_mu = 0, sk_lg_mr = 0, sk_target = 0, sk_direct_max = 0;   // options: geometry of the sketch kernel (0 = default)
    int row_order = 1;                                                     // option: 1 = the first launch of a call takes its rows heaviest first (row_cost_kernel), 0 = in caller order
    int sk_seed_merge = 1; int gk_acsr = 1;                                // option: the general kernel runs on the self-addressed copy too when the graph is large (0 = packed CSR + indptr)
    int64_t est_level_edges = 0;                                           // option: edges per level the first-launch slabs are sized for (0 = automatic)
    int measure_choice = 1;                                                // 0 = kernel and launch shape from the thresholds alone, never from a calibration
    int max_degree_bits = 31;                                              // most bits of a column word the packed degree may take (0 = plain column ids); set before the first gfpush call, which packs
    int dn_block = 0; int dn_csr_lds = 0;                                  // options of the dense kernel (kernel = 3): threads per workgroup (0 = default; 256, 512, 1024); 1 = indptr + indices are staged into LDS when they fit beside the row state
};

// The running estimate of what a row of the recipe needs, with the memory of a recipe the sketch kernel was switched off for.
struct Estimate {
    int kind = 0; int last_kind = 1;                                       // which kernel the running estimate / the last call belongs to
    bool sk_auto_off = false; double sk_off_rmax = 0.0; int sk_off_n_coef = 0;
    bool last_sk_soft = false;                                             // the last call ran the sketch kernel as an automatic or soft pick, not because option kernel = 2 insisted (grow_estimate)
    double edges = 0.0, log = 0.0;                                         // running estimate (grows from the observed maxima)
    double rmax = -1.0; int n_coef = 0;                                    // the call parameters that estimate belongs to
    bool recipe_changed = false;                                           // (the observed maxima on the device belong to the old recipe: the next call clears them)
    double cur_edges = 0.0, cur_log = 0.0;                                 // the estimate the last planned call runs with
    int64_t last_call_rows = 0; bool grown_for_call = true;
};

// ------------------------------------------------------------------ slab capacities

// One set of per-workgroup scratch slabs (all caps are per workgroup).
struct SlabCaps {
    int n_wg = 0;
    cap_t push_cap = 0, resg_cap = 0, log_cap = 0, cand_cap = 0, bucket_cap = 0, bt_cap = 0;
    // sketch kernel (arch_cap > 0): its log record is (column word, 16-bit pusher number) -- log_val is not allocated -- and every
    // pusher of the row leaves coef * share in `arch`
    cap_t arch_cap = 0;
    size_t log_bytes() const { return arch_cap ? 6 * (size_t)log_cap + 8 * (size_t)arch_cap : 12 * (size_t)log_cap; }
    size_t per_wg() const { return 16 * (size_t)(2 * push_cap + resg_cap + cand_cap + bucket_cap) + log_bytes() + 8 * (size_t)bt_cap + 64; }
    bool covers(const SlabCaps& o) const {
        if (o.n_wg == 0) return true;                                  // nothing is asked for
        return n_wg >= o.n_wg && push_cap >= o.push_cap && resg_cap >= o.resg_cap && log_cap >= o.log_cap &&
               cand_cap >= o.cand_cap && bucket_cap >= o.bucket_cap && bt_cap >= o.bt_cap && arch_cap >= o.arch_cap && (arch_cap != 0) == (o.arch_cap != 0);
    }
    // the larger of two layouts of the same kind, field by field (a workspace that has served one recipe keeps serving it
    // when it is re-allocated for another: calls that alternate between recipes must not re-allocate every time -- ADVICE r4)
    void widen(const SlabCaps& o) {
        if (o.n_wg == 0 || (n_wg != 0 && (arch_cap != 0) != (o.arch_cap != 0))) return;
        n_wg = std::max(n_wg, o.n_wg); push_cap = std::max(push_cap, o.push_cap); resg_cap = std::max(resg_cap, o.resg_cap);
        log_cap = std::max(log_cap, o.log_cap); cand_cap = std::max(cand_cap, o.cand_cap); bucket_cap = std::max(bucket_cap, o.bucket_cap);
        bt_cap = std::max(bt_cap, o.bt_cap); arch_cap = std::max(arch_cap, o.arch_cap);
    }
};

// Where the arrays of `wgs` workgroups' slabs start in one allocation (kAbsent: the kind has no such array), and the bytes used.
struct SlabOffsets {
    static constexpr size_t kAbsent = ~(size_t)0;
    size_t push = 0, resg = 0, cand = 0, bucket = 0, arch = kAbsent, log_val = kAbsent, log_key = 0, bt = 0, log_pu = kAbsent, bytes = 0;
};
inline SlabOffsets carve_offsets(const SlabCaps& c, int wgs) {
    SlabOffsets o;
    size_t q = 0;
    o.push = q;    q += 16 * (size_t)wgs * 2 * c.push_cap;
    o.resg = q;    q += 16 * (size_t)wgs * c.resg_cap;
    o.cand = q;    q += 16 * (size_t)wgs * c.cand_cap;
    o.bucket = q;  q += 16 * (size_t)wgs * c.bucket_cap;
    if (c.arch_cap) { o.arch = q; q += 8 * (size_t)wgs * c.arch_cap; }
    else            { o.log_val = q; q += 8 * (size_t)wgs * c.log_cap; }
    o.log_key = q; q += 4 * (size_t)wgs * c.log_cap;
    o.bt = q;      q += 4 * (size_t)wgs * 2 * c.bt_cap;
    if (c.arch_cap) { o.log_pu = q; q += 2 * (size_t)wgs * c.log_cap; }
    o.bytes = (q + 255) & ~(size_t)255;
    return o;
}

// Per-workgroup slab sizes for levels of up to `e_max` edges each (and `log_records` reserve-log records per row; 0 =
// the bound that follows from e_max).  With e_max = the rigorous bound this is the worst case:
// the residue mass of a level never exceeds 1.0 (up to fp64 rounding) and a pushed node has deg <= r/rmax, so the degrees
// pushed in one level sum to <= 1/rmax; the 0.1 % + 16 slack covers the rounding.
//   E_max  = edges traversed in one level  <= min(nnz, 1.001/rmax + 16)
//   F_max  = frontier size of one level    <= min(N, E_max) + 1          (+1: dangling -> seed)
//   reserve-log records of a row           <= (L+1) * F_max
//   support of the reserve map             <= min(N, 1 + L*F_max)
inline double level_edge_bound_of(int64_t nnz) { return (double)nnz + 16.0; }     // no level traverses more than every stored entry

inline SlabCaps slab_sizes(const KernelConsts& kc, int64_t n_nodes, int64_t nnz, int n_coef, double e_max, double log_records) {
    const double n_d = (double)n_nodes;
    const double f_max = std::min(n_d, e_max) + 1.0;
    const double L = (double)(n_coef - 1);
    double logn = (L + 1.0) * f_max + 64.0;
    if (log_records > 0.0) logn = std::min(logn, log_records + 64.0);
    const double supp = std::max(1.0, std::min(std::min(n_d, 1.0 + L * f_max), logn));
    SlabCaps sl;
    sl.resg_cap = (cap_t)std::max(2048.0, 2.0 * f_max);
    sl.log_cap = ((cap_t)logn + 3) & ~3ull;
    sl.cand_cap = (cap_t)supp + 1;
    sl.push_cap = (cap_t)(f_max + 2.0);                        // one entry per pushing node
    // one boundary-table word per 64 edges of a level.  Cheap (1/16 byte per edge), so it is sized well beyond the estimate:
    // a level that outgrows e_max edges but not the entry / log capacities must not send its row to the retry launch
    const double e_bt = std::min(level_edge_bound_of(nnz), std::max(8.0 * e_max, 1048576.0));
    sl.bt_cap = (((cap_t)std::max(e_max, e_bt) >> kc.unit_shift) + 4) & ~1ull;
    sl.bucket_cap = (cap_t)e_max + 2;                 // (key, share) records of one bucketed level
    return sl;
}

// The sketch kernel's slab: two push lists, two boundary tables and the per-EDGE reserve log (`log_records` = edges of a row).
inline SlabCaps sk_slab_sizes(const KernelConsts& kc, int64_t n_nodes, int64_t nnz, double e_max, double log_records, bool at_bound) {
    SlabCaps sl;
    sl.log_cap = ((cap_t)std::min(log_records + 64.0, 4.0e9) + 3) & ~3ull;     // (log positions are 32-bit words in the kernel: a row with more records outgrows its slab and is retried)
    // one entry per pushing node: a few per cent of a level's edges on the graphs the estimate is for (a level with more: general
    // kernel); every node of the level when the slabs are sized from the bound anyway (small graphs)
    sl.push_cap = (cap_t)(std::min((double)n_nodes, at_bound ? e_max : std::max(e_max / 4.0, 4096.0)) + 2.0);
    const double e_bt = std::min(level_edge_bound_of(nnz), std::max(8.0 * e_max, 1048576.0));
    sl.bt_cap = (((cap_t)std::max(e_max, e_bt) >> kc.unit_shift) + 4) & ~1ull;
    // one coef * share per pusher of the ROW (and per level one for the mass dangling nodes return): a few per cent of its edges
    // where this kernel is chosen; pusher numbers are 16 bits in the log, a row with more goes to the general kernel
    sl.arch_cap = (cap_t)std::min((double)kc.sk_max_pushers, std::max(at_bound ? (double)sl.log_cap : (double)sl.log_cap / 4.0, 4096.0));
    sl.arch_cap = (sl.arch_cap + 3) & ~3ull;
    return sl;
}

inline double level_edge_bound(int64_t nnz, double rmax) {
    double e = (double)nnz;
    if (rmax > 0.0) e = std::min(e, std::floor(1.001 / rmax) + 16.0);
    return e;
}

// ------------------------------------------------------------------ the workspace plan

// The workspace a handle holds (have == false: none).
struct Held { bool have = false; SlabCaps est, skl, big; int64_t retry_cap = 0; size_t bytes = 0; };

struct WorkspacePlan {
    // sketch kernel: every workgroup (n_wg == 0: not in use) | general kernel: slabs sized from an estimate of a row's needs |
    // last launch: a few workgroups, slabs sized from the rigorous bounds (n_wg == 0: not needed).  When the held workspace does
    // not fit, these are the layout to allocate: widened by what is held, while both fit the budget.
    SlabCaps est, skl, big;
    bool fits = false;                         // the held workspace serves the call as it is
    int64_t retry_cap = 0; size_t total = 0;   // !fits: rows the per-row lists of the new allocation hold, and its bytes
};

// never plan beyond what the device can give right now: our own cached workspace counts as free
inline size_t workspace_budget(int64_t workspace_mb, bool have_free, size_t free_bytes, size_t held_bytes) {
    size_t budget = (size_t)workspace_mb << 20;
    if (have_free) budget = std::min(budget, (size_t)(0.9 * (double)(free_bytes + held_bytes)));
    return budget;
}

// Workspace policy.  Sizing every workgroup's slab from the 1/rmax bound does not scale: the Cora recipe's
// rmax 1e-7 on a large graph asks for ~2 GB per workgroup, and a fixed budget then silently cut the launch to a few dozen
// workgroups.  Now ALL resident workgroups get a slab sized for what rows of this graph and recipe actually need -- an
// estimate that starts at max(32 Ki edges per level, bound / 4), is capped so that the slabs fit HALF the budget, and grows
// from the maxima the kernel observes -- and a handful of workgroups of a second launch hold bound-sized slabs for the rows
// that outgrow the estimate (they are detected exactly as before and moved to a retry list instead of failing).
// sk_wg > 0: the sketch kernel runs the call on sk_wg workgroups (own, smaller slabs: no HBM residue table, no candidate /
// bucket buffers); the general kernel then only re-runs the rows handed back, on n_wg workgroups.
inline Status plan_workspace(const KernelConsts& kc, int64_t n_nodes, int64_t nnz, int n_coef, double rmax, int n_wg, int sk_wg,
                             int64_t n_seeds, size_t budget, int64_t est_level_edges, Estimate& e, const Held& held,
                             WorkspacePlan& out, std::string& err) {
    const double bound = level_edge_bound(nnz, rmax);
    {
        const SlabCaps worst = slab_sizes(kc, n_nodes, nnz, n_coef, bound, 0.0);
        if (2.0 * (double)worst.resg_cap > 8.0e9 || (double)worst.log_cap > 4.0e9) {
            char buf[160];
            std::snprintf(buf, sizeof buf, "workspace bound exceeds 32-bit record space (order %d, rmax %g)", n_coef - 1, rmax);
            err = buf;
            return kInvalidArg;
        }
    }
    const int kind = sk_wg > 0 ? 2 : 1;
    if (e.rmax != rmax || e.n_coef != n_coef || e.kind != kind) {   // a new recipe (or the other kernel, whose log counts edges): forget the running estimate
        e.rmax = rmax; e.n_coef = n_coef; e.kind = kind; e.edges = 0.0; e.log = 0.0;
        e.recipe_changed = true;                                    // (the observed maxima on the device belong to the old recipe)
    }
    double e_est = est_level_edges > 0 ? (double)est_level_edges
                                       : std::max(e.edges, std::max(32768.0, bound / 4.0));
    e_est = std::min(e_est, bound);
    double log_est = e_est >= bound ? 0.0 : std::max(e.log, 4.0 * e_est);
    SlabCaps est, skl;
    auto plan = [&]() {
        est = slab_sizes(kc, n_nodes, nnz, n_coef, e_est, log_est);
        if (sk_wg > 0) skl = sk_slab_sizes(kc, n_nodes, nnz, e_est, log_est > 0.0 ? log_est : (double)n_coef * e_est, !(log_est > 0.0));
        return (double)est.per_wg() * n_wg + (sk_wg > 0 ? (double)skl.per_wg() * sk_wg : 0.0);
    };
    while (plan() > 0.5 * (double)budget && e_est > 4096.0) {        // shrink the slabs, not the launch
        e_est *= 0.75; log_est = std::max(4096.0, 0.75 * (log_est > 0.0 ? log_est : (double)est.log_cap));
    }
    if (plan() > 0.5 * (double)budget) {
        // (the caller re-plans with the general kernel alone unless option kernel = 2 insists)
        if (sk_wg > 0) { err = "workspace_mb too small for the sketch kernel's slabs"; return kNoMem; }
        n_wg = (int)std::max<size_t>(1, budget / 2 / est.per_wg());
    }
    e.cur_edges = e_est; e.cur_log = log_est;
    est.n_wg = n_wg; skl.n_wg = sk_wg;
    SlabCaps big;                                                    // needed only if the estimate is below the bound
    if (e_est < bound || log_est > 0.0) {
        big = slab_sizes(kc, n_nodes, nnz, n_coef, bound, 0.0);
        const size_t used = est.per_wg() * (size_t)n_wg + skl.per_wg() * (size_t)sk_wg;
        const size_t left = budget - std::min(budget, used);
        int nb = (int)std::min<size_t>(8, left / std::max<size_t>(1, big.per_wg()));
        if (nb < 1) {                                                // not even one worst-case slab fits: give it what is left
            double e_big = bound;
            while (e_big > e_est && slab_sizes(kc, n_nodes, nnz, n_coef, e_big, 0.0).per_wg() > left) e_big *= 0.8;
            big = slab_sizes(kc, n_nodes, nnz, n_coef, std::max(e_big, e_est), 0.0);
            nb = 1;
        }
        big.n_wg = std::min(nb, n_wg);
    }

    out.fits = held.have && held.est.covers(est) && held.big.covers(big) && held.skl.covers(skl) && held.retry_cap >= n_seeds;
    if (!out.fits) {
        auto bytes_of = [&](const SlabCaps& a, const SlabCaps& b, const SlabCaps& c) {
            return a.per_wg() * (size_t)a.n_wg + b.per_wg() * (size_t)b.n_wg + c.per_wg() * (size_t)c.n_wg;
        };
        if (held.have) {                                             // keep what the previous recipes needed, while both fit the budget
            SlabCaps e2 = est, b2 = big, s2 = skl;
            e2.widen(held.est); b2.widen(held.big); s2.widen(held.skl);
            n_seeds = std::max<int64_t>(n_seeds, held.retry_cap);
            if (bytes_of(e2, b2, s2) <= budget) { est = e2; big = b2; skl = s2; }
        }
        out.total = bytes_of(est, big, skl) + 13 * (size_t)std::max<int64_t>(n_seeds, 1) + 3 * 4096 + 1024;   // (per row: two retry lists, order, cost_cls)
        out.retry_cap = std::max<int64_t>(n_seeds, 1);
    }
    out.est = est; out.skl = skl; out.big = big;
    return kOk;
}

// What a handle holds once the shell has applied `p` (it allocates only when the held workspace does not fit).
inline Held held_after(const Held& held, const WorkspacePlan& p) {
    if (p.fits) return held;
    Held h; h.have = true; h.est = p.est; h.skl = p.skl; h.big = p.big; h.retry_cap = p.retry_cap; h.bytes = p.total;
    return h;
}

// Slab sizing follows the RETRY RATE, not the largest row ever seen (sizing 768 slabs for 1.5 x the maximum made a
// 13.6 GB workspace of which a row touches 0.4 MB).  The estimate starts at max(32 Ki edges per level, bound / 4) and grows by
// half when more than 0.1 % of a completed call's rows outgrew their slab (they were re-run exactly by the next launch), and
// doubles above 2 %.  Called when the previous call is known to have completed; applied once per call (grown_for_call is false
// from the moment a call is enqueued until its counters have been looked at).
// Of the finished call: rows_n rows, `outgrown` of them outgrew their slab, `handed_back` went to the retry list.
inline void grow_estimate(Estimate& e, int64_t est_level_edges, int64_t rows_n, double outgrown, double handed_back) {
    if (est_level_edges != 0 || e.grown_for_call || rows_n <= 0) return;
    e.grown_for_call = true;
    if (e.last_kind == 3) return;                                      // (the dense kernel used no slab: nothing to grow from)
    const double rows = (double)rows_n;
    if (outgrown > 0.02 * rows) e.edges = std::max(e.edges, 2.0 * e.cur_edges);
    else if (outgrown > 0.001 * rows) e.edges = std::max(e.edges, 1.5 * e.cur_edges);
    if (outgrown > 0.001 * rows && e.cur_log > 0.0) e.log = std::max(e.log, 1.5 * e.cur_log);
    // the automatic choice of the sketch kernel is a guess from (rmax, graph size): when a call hands more than 5 % of its rows
    // back for other reasons than slab size -- each of them runs twice, the second time on an eighth of the chip -- later calls
    // of this recipe go to the general kernel
    if (e.last_kind == 2 && e.last_sk_soft && handed_back - outgrown > 0.05 * rows) {
        e.sk_auto_off = true; e.sk_off_rmax = e.rmax; e.sk_off_n_coef = e.n_coef;
    }
}

// ------------------------------------------------------------------ kernel and shape

// What a call is asked to run: built from the handle's options or from the recipe's measured Choice, and for each candidate of
// a calibration.  The plan takes kernel, shape and softness from here, never from the handle.
struct Shape {
    int kernel = 0;                          // 0 = the thresholds choose, 1 = general kernel, 2 = sketch kernel whenever the call allows it
    int block_threads = 0, lds_bytes = 0;    // launch shape of the general kernel (0 = choose)
    bool soft = false;                       // kernel 2 is CHOSEN, not insisted on: where the sketch kernel cannot run or keeps handing rows back, the general kernel takes over as in the automatic path
    bool insists_on_sketch() const { return kernel == 2 && !soft; }
};

// Geometry.  Two 512-thread workgroups per CU (80 KB of LDS each) or one 1024-thread workgroup owning all
// 160 KB.  All waves of a workgroup move through a row's phases together, so they wait for memory together
// and compete for issue slots together; a second, independent workgroup on the CU fills those gaps (one
// row's barriers, memory stalls and TOP-K overlap the other row's inserts).  The half-size table costs extra
// hash partitions on the biggest levels, which the one-lane-per-edge EXPAND made cheap (a partition pass
// re-reads and filters at ~25 wave-instructions per 64 edges).  Measured on MI355X, 65 536 rows (tools/exp_run2.sh):
// MAG-shape +13 %, Reddit-shape +15 %, Pubmed +20 %, Cora +74 %; the Amazon2M recipe (rmax 1e-6: levels of
// ~100 k edges, 14+ partitions even with 160 KB) loses 36 % and keeps 1 x 1024, as does any rmax < 5e-6 on a
// graph that is neither tiny nor sparse.
// Three 512-thread workgroups per CU (52 KB of LDS each, 6 waves per SIMD at 80 VGPRs): a third resident row hides
// more of each row's barriers and latency than the smaller table costs in extra hash partitions, once TOP-K no
// longer falls off a cliff at that size (its histogram and tie bucket now live inside the aggregation table's bytes
// and tau is read off a 16x finer histogram).  Measured on MI355X (round 3, 65 536 rows) against 2 x 768 x 80 KB:
// MAG-shape +2.9 %, Reddit-shape +1.3 %, Pubmed +13 %, Cora +10 %.  K > 128 keeps 2 x 768 (sel[K] eats the table).
// The threshold pick of the general kernel's shape, as workgroups per CU: 3, 2 or 1 (general_shape gives their threads and LDS).
inline int threshold_wgs_per_cu(const KernelConsts& kc, int64_t n_nodes, int64_t nnz, double rmax, int K) {
    const bool tiny = (double)n_nodes <= 0.75 * (double)((80 * 1024 - kc.ctl_bytes) / 12);
    const bool sparse = nnz < 8 * n_nodes;
    const bool two_per_cu = K <= 256 && (tiny || sparse || rmax >= 5e-6);
    return !two_per_cu ? 1 : K <= 128 ? 3 : 2;
}

// The threshold pick of the kernel -- the sketch kernel for the recipes whose push test filters (rmax >= 5e-6; at 1e-6 and
// below most of a frontier pushes and the sketch has nothing to remove) on large graphs (measured, 65 536 rows: MAG-shape
// +15 %, Reddit-shape +36 % over the general kernel; the 19.7 k-node Pubmed graph, where half of a frontier pushes, -18 %)
inline bool threshold_picks_sketch(int64_t n_nodes, double rmax) { return rmax >= 5e-6 && n_nodes >= 65536; }

// How the sketch kernel runs a call (use == false: it does not) and how the general kernel does, or re-runs what was handed back.
struct SketchPlan { bool use = false; int block = 0, lds = 0, wg = 0; unsigned lg_mu = 0, lg_mr = 0, cx = 0; double coef_sum = 0.0; };
struct GeneralPlan { int block_threads = 0, lds_bytes = 0, n_wg = 0; unsigned lds_slots = 0; };

// ---- which kernel.  The sketch kernel (gfpush_sketch.hpp) keeps exact fp64 accumulators only for the targets that may
// push and reads the top-K off a cumulative upper-bound table; it needs coef >= 0 (upper bounds add up), a recipe that
// fits its control block, and a threshold the fixed-point sketch can resolve.  Rows it cannot finish come back on a
// retry list and the general kernel runs them.  Whether it takes the call, as far as the call, the options and the estimate's
// sketch-off memory say (it runs on the self-addressed CSR: the shell clears p.use when the graph has none); sets p.coef_sum.
inline void sketch_wanted(const KernelConsts& kc, const Options& opt, const Estimate& e, const Shape& shape, int64_t n_nodes,
                          int64_t n_seeds, const double* coef, int n_coef, double rmax, int K, SketchPlan& p) {
    bool ok = shape.kernel != 1 && n_coef <= kc.sk_max_coef && K <= 128 && rmax * 2147483648.0 >= 64.0 && !opt.force_global && !opt.exact_stats &&
              n_seeds > 0;
    for (int i = 0; i < n_coef; ++i) { if (coef[i] < 0.0) ok = false; p.coef_sum += coef[i]; }
    if (!(p.coef_sum < 1.0e6)) ok = false;
    const bool sk_off = e.sk_auto_off && e.sk_off_rmax == rmax && e.sk_off_n_coef == n_coef;   // (this recipe kept handing rows back)
    p.use = ok && (shape.insists_on_sketch() || (!sk_off && (shape.kernel == 2 || threshold_picks_sketch(n_nodes, rmax))));
}

// The sketch kernel's geometry for a call it takes.  Clears p.use where the sizes leave no room for its tables (an error when
// option kernel = 2 insisted on sizes of its own).
inline Status sketch_geometry(const KernelConsts& kc, const Options& opt, const Shape& shape, int K, SketchPlan& p, std::string& err) {
    p.block = opt.sk_block ? opt.sk_block : 768;
    p.lds = p.block == 512 ? kc.three_lds : p.block == 1024 ? 160 * 1024 : 80 * 1024;
    p.lg_mu = (unsigned)(opt.sk_lg_mu ? opt.sk_lg_mu : (p.block == 512 ? 12 : p.block == 1024 ? 14 : 13));
    // the reserve sketch resolves the K-th total when ~4K of its cells are heavy: 2 048 cells for K <= 32 (the MAG recipe: 1 024 / 4 096
    // cells +4 % / +5 % kernel time), 4 096 beyond (the Reddit recipe, K = 64: -5 %; the exact table pays for them with 680 slots)
    p.lg_mr = (unsigned)(opt.sk_lg_mr ? opt.sk_lg_mr : (K > 32 && p.block >= 768 ? 12 : 11));
    const int64_t x_bytes = (int64_t)p.lds - kc.ctl_bytes - (4ll << p.lg_mu) - (4ll << p.lg_mr);
    p.cx = x_bytes > 0 ? (unsigned)(x_bytes / 12) & ~3u : 0u;
    // the exact table, and the aggregation table TOP-K builds over the level sketch + exact table, need >= min_cap slots
    const int64_t ca = ((4ll << p.lg_mu) + 12ll * p.cx - 16ll * ((int64_t)kc.sk_tie + K)) / 12;
    if (p.cx < (unsigned)kc.min_cap || ca < (int64_t)kc.min_cap) {
        if (shape.insists_on_sketch() && (opt.sk_lg_mu || opt.sk_lg_mr)) {
            char buf[160];
            std::snprintf(buf, sizeof buf, "sketch sizes leave no room for the exact table (sk_lg_mu %u, sk_lg_mr %u)", p.lg_mu, p.lg_mr);
            err = buf;
            return kInvalidArg;
        }
        p.use = false;
    }
    return kOk;
}

// Workgroups of a launch: what fits the chip, the option's cap, no more than the call has rows, at least one.
inline int cap_workgroups(int resident, int max_workgroups, int64_t n_seeds) {
    int wg = resident;
    if (max_workgroups > 0) wg = std::min(wg, max_workgroups);
    return (int)std::max<int64_t>(1, std::min<int64_t>(wg, n_seeds));
}

// The general kernel's launch shape at `wgs_per_cu` (automatic shape) or as the call's shape asks, and the top-K fit test.
inline Status general_shape(const KernelConsts& kc, const Shape& shape, int wgs_per_cu, int K, GeneralPlan& p, std::string& err) {
    const bool auto_shape = shape.block_threads == 0 && shape.lds_bytes == 0;
    p.block_threads = shape.block_threads; p.lds_bytes = shape.lds_bytes;
    if (auto_shape) {
        // 12 waves per row: with the phases compiled as separate functions (32-66 VGPRs each) two 768-thread workgroups
        // fit a CU at 80 VGPRs without spilling the loops (round 3: MAG +11 %, Reddit +7 %, Pubmed +3 % over 2 x 512);
        // (direct-indexed tables of small graphs are instantiated for both two-per-CU shapes: Cora +11 % at 768)
        p.block_threads = wgs_per_cu == 3 ? 512 : wgs_per_cu == 2 ? 768 : 1024;
        p.lds_bytes = wgs_per_cu == 3 ? kc.three_lds : wgs_per_cu == 2 ? 80 * 1024 : 160 * 1024;
    } else {
        if (p.block_threads == 0) p.block_threads = 1024;
        if (p.lds_bytes == 0) p.lds_bytes = 160 * 1024;
    }
    p.lds_slots = (unsigned)((p.lds_bytes - kc.ctl_bytes) / 12) & ~3u;     // multiple of 4: 128-bit LDS accesses on both arrays
    // TOP-K carves sel[K] out of the table region and aggregates in what is
    // left; like every LDS table that aggregation table needs >= min_cap slots (home_lds: cap - kProbeSpan)
    const size_t topk_fixed = 16 * (size_t)K;
    const size_t topk_region = std::max<size_t>(12 * (size_t)kc.min_cap, (size_t)kc.topk_bins * 4 + 16 * (size_t)kc.bucket_cap);   // table, or histogram + compacted bucket
    if ((size_t)p.lds_slots * 12 < topk_fixed + topk_region) {
        char buf[160];
        std::snprintf(buf, sizeof buf, "lds_bytes = %d too small for K = %d (top-K needs %zu bytes of LDS)",
                      p.lds_bytes, K, topk_fixed + topk_region + (size_t)kc.ctl_bytes);
        err = buf;
        return kInvalidArg;
    }
    return kOk;
}

// Workgroups of the general kernel that fit a CU, as the shell has queried them so far (0: not yet): [0] in the shape the call
// asks for, [1] .. [3] in the automatic shape of that many workgroups per CU.
struct Occupancy { int general[4] = {0, 0, 0, 0}; };

// The inputs of a call's plan that do not change while it is planned.
struct CallInputs {
    int64_t n_nodes = 0, nnz = 0; int num_cus = 0;
    int n_coef = 0; double rmax = 0.0; int K = 0; int64_t n_seeds = 0;
    size_t budget = 0;
};

// The general kernel's launch shape, its workgroups, and the workspace of the whole call.  Three fall-backs: the sketch
// kernel's slabs do not fit (sk.use is cleared: the general kernel alone), three workgroups per CU -> two, two -> one.
// kNeedOccupancy: the ladder reached a shape whose occupancy `occ` does not hold yet -- p has the shape, *need the index of occ
// to fill; nothing else has changed and the shell calls again.  Otherwise `e` is the estimate after the plan; on kOk `held`
// becomes what the handle holds once the shell has allocated, which it does when *realloc is set (a pass of the ladder that
// did not fit allocates, and the next pass widens what that one would have held -- as when each pass allocated at once).
inline Status plan_general(const KernelConsts& kc, const CallInputs& in, const Options& opt, const Shape& shape, const Occupancy& occ,
                           SketchPlan& sk_io, GeneralPlan& p, Estimate& e_io, Held& held_io, bool* realloc, int* need, std::string& err) {
    SketchPlan sk = sk_io; Estimate e = e_io; Held held = held_io;
    *realloc = false;
    const int K = in.K;
    const bool auto_shape = shape.block_threads == 0 && shape.lds_bytes == 0;
    int wgs_per_cu = auto_shape ? threshold_wgs_per_cu(kc, in.n_nodes, in.nnz, in.rmax, K) : 1;
    for (;;) {
        Status st = general_shape(kc, shape, wgs_per_cu, K, p, err);
        if (st) { e_io = e; return st; }
        const int rung = auto_shape ? wgs_per_cu : 0;
        const int per_cu = occ.general[rung];
        if (per_cu <= 0) { *need = rung; return kNeedOccupancy; }
        p.n_wg = in.num_cus * per_cu;
        if (opt.max_workgroups > 0) p.n_wg = std::min(p.n_wg, opt.max_workgroups);
        if (sk.use) p.n_wg = std::min(p.n_wg, std::max(8, in.num_cus / 2));  // the general kernel only re-runs what the sketch kernel hands back (a per-mille of the call)
        p.n_wg = (int)std::max<int64_t>(1, std::min<int64_t>(p.n_wg, in.n_seeds));
        WorkspacePlan wp;
        st = plan_workspace(kc, in.n_nodes, in.nnz, in.n_coef, in.rmax, p.n_wg, sk.use ? sk.wg : 0, in.n_seeds, in.budget,
                            opt.est_level_edges, e, held, wp, err);
        if (st == kNoMem && sk.use && !shape.insists_on_sketch()) {          // the automatic choice must not fail where the general kernel alone fits
            sk.use = false; err.clear();
            continue;
        }
        if (st) { e_io = e; return st; }
        if (!wp.fits) { held = held_after(held, wp); *realloc = true; }
        if (sk.use) break;
        // the workspace budget could not hold two workgroups per CU: one big workgroup per CU is better than
        // a half-empty chip
        if (wgs_per_cu == 3 && held.est.n_wg < p.n_wg && held.est.n_wg < 3 * in.num_cus) { wgs_per_cu = 2; continue; }
        if (wgs_per_cu == 2 && held.est.n_wg < p.n_wg && held.est.n_wg < 2 * in.num_cus) { wgs_per_cu = 1; continue; }
        break;
    }
    p.n_wg = std::min(p.n_wg, held.est.n_wg);
    sk_io = sk; e_io = e; held_io = held;
    return kOk;
}

// direct-indexed level tables: the whole graph fits the table of the 512-thread kernel (Cora, Citeseer)
inline bool direct_tables(const Options& opt, int64_t n_nodes, const GeneralPlan& gk) {
    return (gk.block_threads == 512 || gk.block_threads == 768) && (cap_t)n_nodes + 4 <= (cap_t)gk.lds_slots && opt.direct_tables;
}
// TOP-K prunes by an upper bound unless the statistics must be exact; the bound needs coef >= 0
inline bool prune_allowed(const Options& opt, const double* coef, int n_coef) {
    bool prune = !opt.exact_stats;
    for (int i = 0; i < n_coef; ++i) if (coef[i] < 0.0) prune = false;
    return prune;
}
// Whether the general kernel runs on the self-addressed copy of the graph, where the graph has one (large graphs; `diag_build`:
// the diagnostic build instruments the general kernel on the packed CSR only).
inline bool general_wants_acsr(bool diag_build, const Options& opt, bool direct, int64_t n_nodes, int64_t n_seeds) {
    return !diag_build && opt.gk_acsr && !direct && !opt.force_global && n_nodes >= 65536 && n_seeds > 0;
}

// ------------------------------------------------------------------ the dense kernel (option kernel = 3)

// The dense kernel (gfpush_dense.hpp) keeps a row's whole state in one workgroup's LDS, indexed by node id over the node count
// rounded up to whole 64-node chunks (one wave's step):
//   [ control block | select histogram | cur f64 | next f64 | reserve f64 | touched marks, one 64-bit word per chunk | indptr | indices ]
// 24 bytes per node + 1 bit, the last two arrays only when the CSR is staged.  TOP-K's list of selected (value, column) pairs
// -- min(K, N) entries of 16 bytes -- lives in cur | next, which are dead by then, so K does not enter the layout.
constexpr int kDenseLds = 163840;              // LDS of a CU: the most one workgroup can own
constexpr int kDenseCtlBytes = 512;            // control block (DenseCtl: the row, the select's state, statistics, coefficients)
constexpr int kDenseHistBytes = 1024;          // 256 bins of the radix select
constexpr int64_t kDenseMaxNodes = 6720;       // the largest multiple of 64 whose state fits: 1536 + 6720 * 24 + 6720 / 8 = 163 656 bytes
static_assert(kDenseCtlBytes + kDenseHistBytes + kDenseMaxNodes * 24 + kDenseMaxNodes / 8 <= kDenseLds &&
              kDenseCtlBytes + kDenseHistBytes + (kDenseMaxNodes + 64) * 24 + (kDenseMaxNodes + 64) / 8 > kDenseLds && kDenseMaxNodes >= 5120,
              "kDenseMaxNodes is the cap the LDS layout gives");

struct DensePlan {
    bool fits = false;                         // the row state fits beside lds_pad (else nothing below is meaningful)
    bool csr_lds = false;                      // indptr + indices are staged into LDS
    int lds_bytes = 0, block = 0, workgroups = 0;
    int64_t n_pad = 0;                         // nodes rounded up to whole chunks: the length of cur / next / reserve
    unsigned off_hist = 0, off_cur = 0, off_next = 0, off_reserve = 0, off_marks = 0, off_indptr = 0, off_indices = 0, state_end = 0;   // byte offsets
};

// The layout and launch shape of a dense-kernel call.  per_cu = workgroups of that shape the shell has measured to fit a CU
// (0: not asked yet -- workgroups stays 0).
inline DensePlan dense_plan(const Options& opt, int64_t n_nodes, int64_t nnz, int K, int lds_pad, int num_cus = 0, int per_cu = 0, int64_t n_seeds = 0) {
    DensePlan d;
    (void)K;
    if (n_nodes < 1 || n_nodes > kDenseMaxNodes || nnz < 0) return d;
    d.n_pad = (n_nodes + 63) & ~(int64_t)63;
    size_t q = (size_t)kDenseCtlBytes;
    d.off_hist = (unsigned)q;    q += (size_t)kDenseHistBytes;
    d.off_cur = (unsigned)q;     q += 8 * (size_t)d.n_pad;
    d.off_next = (unsigned)q;    q += 8 * (size_t)d.n_pad;
    d.off_reserve = (unsigned)q; q += 8 * (size_t)d.n_pad;
    d.off_marks = (unsigned)q;   q += (size_t)d.n_pad / 8;
    d.state_end = (unsigned)q;
    const size_t room = (size_t)kDenseLds - (size_t)std::min(std::max(lds_pad, 0), kDenseLds);
    if (q > room) return d;
    d.fits = true;
    const size_t csr = ((4 * (size_t)(n_nodes + 1) + 7) & ~(size_t)7) + ((4 * (size_t)nnz + 7) & ~(size_t)7);
    if (opt.dn_csr_lds && q + csr <= room) {
        d.csr_lds = true;
        d.off_indptr = (unsigned)q;  q += (4 * (size_t)(n_nodes + 1) + 7) & ~(size_t)7;
        d.off_indices = (unsigned)q; q += (4 * (size_t)nnz + 7) & ~(size_t)7;
    }
    d.lds_bytes = (int)((q + 15) & ~(size_t)15);
    d.block = opt.dn_block ? opt.dn_block : 512;
    if (per_cu > 0) d.workgroups = cap_workgroups(num_cus * per_cu, opt.max_workgroups, n_seeds);
    return d;
}

// Whether the dense kernel takes the call: only when option kernel = 3 asks for it, the graph is within the node cap and its
// state fits the LDS that lds_pad leaves.  Any sign of coef, any n_coef >= 1, K <= 1024 and rmax >= 0 are fine.
inline bool dense_wanted(const Options& opt, int64_t n_nodes, int64_t nnz, int n_coef, double rmax, int K, int lds_pad) {
    if (opt.kernel != 3 || n_nodes < 1 || n_nodes > kDenseMaxNodes) return false;
    if (n_coef < 1 || K < 1 || K > 1024 || !(rmax >= 0.0)) return false;
    return dense_plan(opt, n_nodes, nnz, K, lds_pad).fits;
}

// ------------------------------------------------------------------ measured choice

// Rows timed per candidate / smallest call that is worth a calibration.  16 384 rows are ~30 rows per resident workgroup: both
// kernels LEARN per workgroup how to plan a level (cand_q / ratio_q) and pay for an overflowed pass while they do; on 2 048 rows
// (4 per workgroup) the MAG line's sketch kernel timed 2.0 ms against 1.4 ms for the general kernel in its slowest shape, which
// takes 36 ms against 21 ms on a full call.
constexpr int64_t kCalRows = 16384, kCalMinRows = 32768;

// Measured choice: which kernel and launch shape run a recipe on this graph is decided by timing the
// candidates -- they are exact and interchangeable -- on the first rows of the first large call of the recipe, not by
// thresholds on rmax and graph size.  One entry per (rmax, n_coef, K); ms[] = general kernel in the shape the old
// thresholds pick / sketch kernel / general kernel in the other shape (0: not a candidate).
struct Choice { double rmax; int n_coef, K; int kernel, block_threads, lds_bytes; float ms[3]; };

// A recipe is calibrated, and a measured choice used, only when nothing is forced.
inline bool choice_applies(bool diag_build, const Options& opt, int64_t n_seeds) {
    return !(diag_build || opt.kernel != 0 || opt.block_threads != 0 || opt.lds_bytes != 0 || !opt.measure_choice ||
             opt.force_global || opt.exact_stats || n_seeds <= 0);
}

// the general kernel in the shape the thresholds pick, the sketch kernel, the general kernel in the other shape
inline void choice_candidates(const KernelConsts& kc, int64_t n_nodes, int64_t nnz, double rmax, int K, Shape cands[3]) {
    const bool two_per_cu = threshold_wgs_per_cu(kc, n_nodes, nnz, rmax, K) > 1;
    cands[0] = Shape{1, 0, 0, false}; cands[1] = Shape{2, 0, 0, false};
    cands[2] = two_per_cu ? Shape{1, 1024, 160 * 1024, false} : Shape{1, 768, 80 * 1024, false};
}
inline bool is_candidate(int c, int K) { return !(c == 2 && K > 256); }    // (two workgroups per CU need K <= 256: no other shape to try)

// what the thresholds would pick stays unless another candidate is more than 5 % faster (timing noise must not flip a recipe);
// kernel 0: nothing could be timed -- the thresholds decide, as without a calibration
inline void pick_choice(bool threshold_sketch, const Shape cands[3], Choice& ch) {
    const int heur = threshold_sketch && ch.ms[1] > 0.f ? 1 : 0;
    int pick = ch.ms[heur] > 0.f ? heur : -1;
    for (int c = 0; c < 3; ++c)
        if (ch.ms[c] > 0.f && (pick < 0 || ch.ms[c] < 0.95f * ch.ms[pick])) pick = c;
    if (pick >= 0) { ch.kernel = cands[pick].kernel; ch.block_threads = cands[pick].block_threads; ch.lds_bytes = cands[pick].lds_bytes; }
}

// ------------------------------------------------------------------ the packed output slab and the multi-GPU cut

// One packed slab [val f64 x slots | row i32 x slots | col i32 x slots | filled i32 x rows], slots = rows * K: the layout the
// kernels write a call's rows in for gp_gfpush and the multi-GPU gather (and grand_plus_amd/sharded.py all-gathers).
struct PackedSlab {
    size_t val = 0, row = 0, col = 0, filled = 0;     // byte offsets
    size_t bytes = 0;                                 // of the four arrays
    size_t stride = 0;                                // 16-byte padded: what one GPU contributes to the gather
    PackedSlab(int64_t rows, int K) {
        const size_t slots = (size_t)rows * (size_t)K;
        row = 8 * slots; col = 12 * slots; filled = 16 * slots;
        bytes = filled + 4 * (size_t)rows;
        stride = (bytes + 15) / 16 * 16;
    }
};

// bytes one GPU contributes to the gather: [val f64 | row i32 | col i32 | filled i32] for `per` rows, 16-byte padded
// (the layout of grand_plus_amd/sharded.py:packed_stride, so both multi-GPU drivers move the same slab)
inline size_t packed_stride(int64_t per, int K) { return PackedSlab(per, K).stride; }

// How one call is cut over the GPUs of a multi-GPU handle (pure host arithmetic: gp_internal_multi_plan exposes it to the
// CPU tests, because the >= 2-GPU branch cannot run on a one-GPU box).
//   G   GPUs that compute (1 when the call is too small to shard and no collective is forced)
//   Gc  GPUs that take part in the gather (the whole communicator for the RCCL path, else G)
//   per rows every participant contributes to the gather = ceil(S / G); GPU d computes rows [d per, min((d+1) per, S))
//   single: the call is handed to part[0] as it is (no slab, no gather)
struct MultiPlan { int G = 1, Gc = 1; int64_t per = 0; size_t stride = 0; bool single = true; };
inline MultiPlan plan_multi(int64_t n_seeds, int K, int n_parts, int64_t min_rows_per_gpu, bool force_collective, bool gather_host) {
    MultiPlan m;
    m.G = n_parts;
    if (n_seeds < min_rows_per_gpu * (int64_t)m.G && !force_collective) m.G = 1;       // small calls stay on one GPU
    m.single = m.G == 1 && !force_collective;
    m.per = (n_seeds + m.G - 1) / m.G;
    m.stride = packed_stride(m.per, K);
    m.Gc = gather_host ? m.G : n_parts;                    // the communicator spans every GPU of the handle
    return m;
}
inline void plan_block(const MultiPlan& m, int d, int64_t n_seeds, int64_t* lo, int64_t* n) {
    *lo = std::min<int64_t>((int64_t)d * m.per, n_seeds);
    *n = d < m.G ? std::min<int64_t>(*lo + m.per, n_seeds) - *lo : 0;
}

// ------------------------------------------------------------------ the merge of gp_gfpush

// The rows of gp_gfpush go straight from the kernel into pinned host memory, into one packed slab that starts in a SENTINEL
// pattern -- every byte 0xFF: value NaN, row / column / filled -1, none of which the kernels can write.  Nothing orders a row's
// `filled` word against its slots on the way there, so a row is merged when all of its filled slots have left that pattern in
// all three arrays.
struct MergeState { int64_t first_open = 0, n_merged = 0; };

// Merges every row that has fully arrived since the last sweep into the caller's arrays ("write only v > 0", graph.h:121).
// (the arrival test reads the slab through PLAIN pointers behind a compiler barrier per sweep, so that its loops vectorise: 96
//  volatile loads per row were most of this thread's CPU time, VERDICT r5 #6.  A slot that has left the sentinel pattern never
//  returns to it during the call, so what the test saw is what the copies behind it read.)
inline void merge_sweep(const char* slab, const PackedSlab& lay, int K, int64_t n_seeds, unsigned char* done, MergeState& m,
                        int32_t* row_idx, int32_t* col_idx, double* value) {
    const uint64_t* const p_val = (const uint64_t*)(slab + lay.val); const int* const p_row = (const int*)(slab + lay.row);
    const int* const p_col = (const int*)(slab + lay.col); const volatile int* const h_filled = (const volatile int*)(slab + lay.filled);
    int64_t first_open = m.first_open, n_merged = m.n_merged;
    bool prefix = true;
    asm volatile("" ::: "memory");
    for (int64_t it = first_open; it < n_seeds; ++it) {
        if (done[it]) { if (prefix) first_open = it + 1; continue; }
        const int nf = h_filled[it];
        if (nf < 0 || nf > K) { prefix = false; continue; }
        const int64_t o = it * (int64_t)K;
        if (nf > 0) {
            int lo = 0; uint64_t sent = 0;
            for (int i = 0; i < nf; ++i) { lo |= p_row[o + i] | p_col[o + i]; sent |= (uint64_t)(p_val[o + i] == ~0ull); }     // (a sentinel word is -1: the sign bit of the OR says one is left)
            if (lo < 0 || sent) { prefix = false; continue; }
            std::atomic_thread_fence(std::memory_order_acquire);
            std::memcpy(row_idx + o, p_row + o, sizeof(int) * (size_t)nf);
            std::memcpy(col_idx + o, p_col + o, sizeof(int) * (size_t)nf);
            std::memcpy(value + o, p_val + o, sizeof(double) * (size_t)nf);
        }
        done[it] = 1; ++n_merged;
        if (prefix) first_open = it + 1;
    }
    m.first_open = first_open; m.n_merged = n_merged;
}

// The merge rule -- a row is taken once every filled slot has left the sentinel pattern in all three arrays -- rests on an
// 8-byte value store never arriving torn and on no slot being rewritten after it first arrived.  With
// the launches retired the slab holds the rows as the kernels left them: every row merged WHILE the kernel ran must equal it.
// Returns the rows that do not (*first_bad: the first of them, or -1).
inline int64_t verify_merged(const char* slab, const PackedSlab& lay, int K, int64_t n_seeds, const int32_t* row_idx,
                             const int32_t* col_idx, const double* value, int64_t* first_bad) {
    const volatile uint64_t* h_val = (const volatile uint64_t*)(slab + lay.val); const volatile int* h_row = (const volatile int*)(slab + lay.row);
    const volatile int* h_col = (const volatile int*)(slab + lay.col); const volatile int* h_filled = (const volatile int*)(slab + lay.filled);
    int64_t bad = 0;
    *first_bad = -1;
    for (int64_t it = 0; it < n_seeds; ++it) {
        const int nf = h_filled[it];
        const int64_t o = it * (int64_t)K;
        const bool same = nf >= 0 && nf <= K &&
                          std::memcmp(row_idx + o, (const void*)(h_row + o), sizeof(int) * (size_t)nf) == 0 &&
                          std::memcmp(col_idx + o, (const void*)(h_col + o), sizeof(int) * (size_t)nf) == 0 &&
                          std::memcmp(value + o, (const void*)(h_val + o), sizeof(double) * (size_t)nf) == 0;
        if (!same) { ++bad; if (*first_bad < 0) *first_bad = it; }
    }
    return bad;
}

// The rows of one GPU's gathered slab (`per` rows of K slots; the first n_rows are this call's) into the caller's arrays at row0.
inline void scatter_filled(const char* slab, int64_t per, int K, int64_t row0, int64_t n_rows,
                           int32_t* row_idx, int32_t* col_idx, double* value)
{
    const PackedSlab lay(per, K);
    const double* h_val = (const double*)(slab + lay.val); const int* h_row = (const int*)(slab + lay.row);
    const int* h_col = (const int*)(slab + lay.col); const int* h_filled = (const int*)(slab + lay.filled);
    for (int64_t it = 0; it < n_rows; ++it) {
        const int nf = h_filled[it];
        if (nf <= 0) continue;                             // graph.h:121: only v > 0 slots are written
        const size_t o = (size_t)it * K, oo = (size_t)(row0 + it) * K;
        std::memcpy(row_idx + oo, h_row + o, sizeof(int) * (size_t)nf);
        std::memcpy(col_idx + oo, h_col + o, sizeof(int) * (size_t)nf);
        std::memcpy(value + oo, h_val + o, sizeof(double) * (size_t)nf);
    }
}

}  // namespace planning
}  // namespace gp
