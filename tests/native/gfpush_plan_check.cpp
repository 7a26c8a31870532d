// Stand-alone driver of grand_plus_amd/csrc/gfpush_plan.hpp for tests/test_host_gfpush_plan.py: reads one command per line on
// stdin, prints one line of numbers per decision.  Built with the address and undefined-behaviour sanitizers; no HIP, no GPU.
//
//   consts  ctl_bytes three_lds min_cap topk_bins bucket_cap unit_shift sk_max_pushers sk_max_coef sk_tie
//   handle  n_nodes nnz num_cus acsr_ok          a fresh handle: default options, no estimate, no workspace
//   opt     key value                            gp_set_option's keys
//   occ     sketch general[0] .. general[3]      workgroups per CU the shell would be told (0: unknown -> an error here)
//   call    n_coef rmax K rows coef...           plans the call as gfpush.hip's enqueue_call does and books it as enqueued
//   ws      n_coef rmax n_wg sk_wg rows budget   plan_workspace alone on the handle's estimate and held workspace (applied)
//   est     field value                          sets a field of the running estimate
//   grow    rows outgrown handed_back            grow_estimate
//   pick    rmax K ms0 ms1 ms2                   the candidate list and the 5 % rule
//   selftest                                     slab layouts at the edges, covers / widen, the merge, verify, scatter
#include "gfpush_plan.hpp"

#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <vector>

using namespace gp::planning;

namespace {

KernelConsts kc;
struct Handle { int64_t n_nodes = 0, nnz = 0; int num_cus = 0; bool acsr_ok = true; Options opt; Estimate est; Held held; } h;
int occ_sketch = 0; Occupancy occ;

// The arrays of one carved slab set are in order, disjoint, inside the bytes reported, and every array (and every workgroup's
// part of an array that is accessed 16 bytes at a time: 16-byte records, log_val / arch doubles, log_key, bt) starts 16-byte aligned.
bool layout_ok(const SlabCaps& c, int wgs, std::string& why) {
    const SlabOffsets o = carve_offsets(c, wgs);
    struct Arr { const char* name; size_t off, per_wg; };
    std::vector<Arr> arrs = {{"push", o.push, 32 * (size_t)c.push_cap}, {"resg", o.resg, 16 * (size_t)c.resg_cap},
                             {"cand", o.cand, 16 * (size_t)c.cand_cap}, {"bucket", o.bucket, 16 * (size_t)c.bucket_cap}};
    if (c.arch_cap) arrs.push_back({"arch", o.arch, 8 * (size_t)c.arch_cap}); else arrs.push_back({"log_val", o.log_val, 8 * (size_t)c.log_cap});
    arrs.push_back({"log_key", o.log_key, 4 * (size_t)c.log_cap});
    arrs.push_back({"bt", o.bt, 8 * (size_t)c.bt_cap});
    if ((c.arch_cap != 0) != (o.log_pu != SlabOffsets::kAbsent) || (c.arch_cap != 0) != (o.arch != SlabOffsets::kAbsent) ||
        (c.arch_cap == 0) != (o.log_val != SlabOffsets::kAbsent)) { why = "kind"; return false; }
    size_t end = 0;
    for (const Arr& a : arrs) {
        if (a.off == SlabOffsets::kAbsent || a.off < end) { why = std::string(a.name) + " overlaps"; return false; }
        if (a.off % 16 || a.per_wg % 16) { why = std::string(a.name) + " misaligned"; return false; }
        end = a.off + a.per_wg * (size_t)wgs;
    }
    if (c.arch_cap) {
        if (o.log_pu < end || o.log_pu % 16) { why = "log_pu"; return false; }
        end = o.log_pu + 2 * (size_t)c.log_cap * (size_t)wgs;
    }
    if (end > o.bytes || o.bytes % 256) { why = "bytes"; return false; }
    if (o.bytes > ((c.per_wg() * (size_t)wgs + 255) & ~(size_t)255)) { why = "per_wg"; return false; }     // what the plan adds up covers what carve hands out
    return true;
}

// A whole workspace as the shell carves it: skl | est | big | the per-row lists, inside `total`.
bool workspace_ok(const Held& w, std::string& why) {
    size_t p = 0;
    if (w.skl.n_wg > 0) { if (!layout_ok(w.skl, w.skl.n_wg, why)) return false; p += carve_offsets(w.skl, w.skl.n_wg).bytes; }
    if (!layout_ok(w.est, w.est.n_wg, why)) return false;
    p += carve_offsets(w.est, w.est.n_wg).bytes;
    if (w.big.n_wg > 0) { if (!layout_ok(w.big, w.big.n_wg, why)) return false; p += carve_offsets(w.big, w.big.n_wg).bytes; }
    // two retry lists and the order (u32 each), the cost classes (a byte each), then order_hist[64] at the next 256-byte boundary
    const size_t lists = p + 13 * (size_t)w.retry_cap;
    const size_t hist = (lists + 255) & ~(size_t)255;
    if (hist + 64 * 4 > w.bytes) { why = "lists"; return false; }
    return true;
}

bool set_option(const std::string& k, int64_t v) {
    Options& o = h.opt;
    struct { const char* key; int* p; } ints[] = {
        {"block_threads", &o.block_threads}, {"lds_bytes", &o.lds_bytes}, {"lds_pad", &o.lds_pad}, {"kernel", &o.kernel},
        {"sk_block_threads", &o.sk_block}, {"sk_lg_mu", &o.sk_lg_mu}, {"sk_lg_mr", &o.sk_lg_mr}, {"sk_direct_max", &o.sk_direct_max},
        {"sk_seed_merge", &o.sk_seed_merge}, {"row_order", &o.row_order}, {"gk_acsr", &o.gk_acsr}, {"sk_target", &o.sk_target},
        {"measure_choice", &o.measure_choice}, {"verify_merge", &o.verify_merge}, {"pretouch", &o.pretouch},
        {"max_workgroups", &o.max_workgroups}, {"force_global", &o.force_global}, {"exact_stats", &o.exact_stats},
        {"direct_tables", &o.direct_tables}, {"solo_levels", &o.solo_levels}, {"seedrow", &o.seedrow}, {"diag_flags", &o.diag_flags},
        {"max_degree_bits", &o.max_degree_bits}};
    for (auto& e : ints) if (k == e.key) { *e.p = (int)v; return true; }
    if (k == "workspace_mb") { o.workspace_mb = v; return true; }
    if (k == "est_level_edges") { o.est_level_edges = v; return true; }
    return false;
}

bool set_estimate(const std::string& k, double v) {
    Estimate& e = h.est;
    if (k == "kind") e.kind = (int)v; else if (k == "last_kind") e.last_kind = (int)v; else if (k == "sk_auto_off") e.sk_auto_off = v != 0;
    else if (k == "last_sk_soft") e.last_sk_soft = v != 0; else if (k == "edges") e.edges = v; else if (k == "log") e.log = v;
    else if (k == "rmax") e.rmax = v; else if (k == "n_coef") e.n_coef = (int)v; else if (k == "cur_edges") e.cur_edges = v;
    else if (k == "cur_log") e.cur_log = v; else if (k == "last_call_rows") e.last_call_rows = (int64_t)v;
    else if (k == "grown_for_call") e.grown_for_call = v != 0; else if (k == "recipe_changed") e.recipe_changed = v != 0;
    else return false;
    return true;
}

void print_estimate(const char* tag) {
    const Estimate& e = h.est;
    std::printf("%s %.17g %.17g %.17g %.17g %d %d %d %.17g %d\n", tag, e.edges, e.log, e.cur_edges, e.cur_log, (int)e.recipe_changed,
                (int)e.grown_for_call, (int)e.sk_auto_off, e.sk_off_rmax, e.sk_off_n_coef);
}

// One call, planned as enqueue_call plans it and booked as enqueued.
void do_call(int n_coef, double rmax, int K, int64_t rows, const std::vector<double>& coef) {
    const Shape shape{h.opt.kernel, h.opt.block_threads, h.opt.lds_bytes, false};
    SketchPlan sk; GeneralPlan gk;
    std::string err;
    sketch_wanted(kc, h.opt, h.est, shape, h.n_nodes, rows, coef.data(), n_coef, rmax, K, sk);
    if (sk.use && !h.acsr_ok) sk.use = false;
    Status st = kOk;
    if (sk.use) st = sketch_geometry(kc, h.opt, shape, K, sk, err);
    if (!st && sk.use) sk.wg = cap_workgroups(h.num_cus * occ_sketch, h.opt.max_workgroups, rows);
    bool realloc = false; int passes = 0;
    if (!st) {
        CallInputs in;
        in.n_nodes = h.n_nodes; in.nnz = h.nnz; in.num_cus = h.num_cus; in.n_coef = n_coef; in.rmax = rmax; in.K = K; in.n_seeds = rows;
        in.budget = workspace_budget(h.opt.workspace_mb, false, 0, h.held.bytes);
        Occupancy known;                                   // filled shape by shape, as the shell queries them
        int need = 0;
        while ((st = plan_general(kc, in, h.opt, shape, known, sk, gk, h.est, h.held, &realloc, &need, err)) == kNeedOccupancy) {
            known.general[need] = occ.general[need];
            ++passes;
            if (known.general[need] <= 0) { st = kInvalidArg; err = "occupancy of this shape was not recorded"; break; }
        }
    }
    std::string why = "-";
    const bool lay = st || workspace_ok(h.held, why);
    if (!st) {
        h.est.recipe_changed = false;
        h.est.last_call_rows = rows; h.est.grown_for_call = false;
        h.est.last_kind = sk.use ? 2 : 1; h.est.last_sk_soft = sk.use && !shape.insists_on_sketch();
    }
    std::printf("plan %d %d %d %d %d %d %lld %d %d %d %d %d %d %.17g %.17g %s|%s\n", (int)st, sk.use ? 2 : 1, sk.use ? sk.wg : gk.n_wg,
                sk.use ? sk.block : gk.block_threads, sk.use ? sk.lds : gk.lds_bytes, sk.use ? (int)sk.cx : (int)gk.lds_slots,
                (long long)h.held.bytes, (int)lay, (int)realloc, passes, h.held.est.n_wg, h.held.big.n_wg, h.held.skl.n_wg,
                h.est.cur_edges, h.est.cur_log, why.c_str(), err.c_str());
}

void do_ws(int n_coef, double rmax, int n_wg, int sk_wg, int64_t rows, size_t budget) {
    WorkspacePlan wp; std::string err, why = "-";
    const Status st = plan_workspace(kc, h.n_nodes, h.nnz, n_coef, rmax, n_wg, sk_wg, rows, budget, h.opt.est_level_edges, h.est, h.held, wp, err);
    bool lay = true;
    if (!st) { h.held = held_after(h.held, wp); lay = workspace_ok(h.held, why); }
    const double bound = level_edge_bound(h.nnz, rmax);
    std::printf("ws %d %d %d %d %d %zu %zu %zu %zu %d %.17g %.17g %.17g %d %llu %s|%s\n", (int)st, wp.est.n_wg, wp.big.n_wg, wp.skl.n_wg, (int)wp.fits,
                wp.total, wp.est.per_wg(), wp.big.per_wg(), wp.skl.per_wg(), (int)lay, h.est.cur_edges, h.est.cur_log, bound,
                (int)h.est.recipe_changed, (unsigned long long)slab_sizes(kc, h.n_nodes, h.nnz, n_coef, bound, 0.0).per_wg(), why.c_str(), err.c_str());
}

// ---------------------------------------------------------------- self tests
int n_fail = 0;
void check(bool ok, const char* name) { std::printf("%s %s\n", ok ? "PASS" : "FAIL", name); if (!ok) ++n_fail; }

void test_slabs() {
    std::string why;
    const SlabCaps gen = slab_sizes(kc, 100000, 1500000, 11, 32768.0, 131072.0);
    const SlabCaps skl = sk_slab_sizes(kc, 100000, 1500000, 32768.0, 131072.0, false);
    const SlabCaps skb = sk_slab_sizes(kc, 2000, 17000, 10016.0, 5 * 10016.0, true);
    check(gen.arch_cap == 0 && skl.arch_cap > 0 && skb.arch_cap > 0, "slab_kinds");
    check(layout_ok(gen, 1, why) && layout_ok(gen, 768, why) && layout_ok(gen, 3, why), "layout_general");
    check(layout_ok(skl, 1, why) && layout_ok(skl, 512, why) && layout_ok(skb, 7, why), "layout_sketch");
    check(layout_ok(gen, 0, why) && carve_offsets(gen, 0).bytes == 0 && layout_ok(SlabCaps(), 0, why), "layout_zero_workgroups");
    // covers(a, b) holds after a.widen(b), for layouts of one kind
    SlabCaps a = slab_sizes(kc, 100000, 1500000, 5, 4096.0, 0.0), b = gen;
    a.n_wg = 768; b.n_wg = 128;
    const bool before = a.covers(b);
    a.widen(b);
    check(!before && a.covers(b) && a.n_wg == 768 && a.log_cap == std::max(gen.log_cap, a.log_cap) && layout_ok(a, a.n_wg, why), "widen_then_covers");
    SlabCaps s1 = skl, s2 = skb; s1.n_wg = 4; s2.n_wg = 9; s1.widen(s2);
    check(s1.covers(s2) && s1.covers(skl) && s1.n_wg == 9, "widen_then_covers_sketch");
    // widen across kinds leaves a as it was (and such a layout never covers the other kind)
    SlabCaps g2 = gen; g2.n_wg = 5; const SlabCaps keep = g2; SlabCaps k2 = skl; k2.n_wg = 600;
    g2.widen(k2);
    check(std::memcmp(&g2, &keep, sizeof keep) == 0 && !g2.covers(k2), "widen_across_kinds");
    SlabCaps none; none.widen(k2);                          // (nothing held yet: takes the other's layout)
    check(none.covers(k2) && none.arch_cap == k2.arch_cap, "widen_empty");
    SlabCaps zero = gen; zero.n_wg = 0;
    check(SlabCaps().covers(zero) && keep.covers(zero), "covers_nothing_asked");
}

// A slab in the sentinel pattern with 3 rows, K = 4, filled counts 0, 2, 4; the words arrive in stages, a sweep after each.
void test_merge() {
    const int K = 4; const int64_t n = 3;
    const PackedSlab lay(n, K);
    check(lay.val == 0 && lay.row == 8 * 12 && lay.col == 12 * 12 && lay.filled == 16 * 12 && lay.bytes == 16 * 12 + 12 && lay.stride == 208 &&
          packed_stride(n, K) == 208 && packed_stride(5, 3) == ((size_t)16 * 5 * 3 + 4 * 5 + 15) / 16 * 16, "packed_layout");
    std::vector<char> slab(lay.bytes, (char)0xFF);
    double* val = (double*)(slab.data() + lay.val); int* row = (int*)(slab.data() + lay.row);
    int* col = (int*)(slab.data() + lay.col); int* filled = (int*)(slab.data() + lay.filled);
    std::vector<int32_t> out_row(n * K, 0x11111111), out_col(n * K, 0x22222222); std::vector<double> out_val(n * K, -7.5);
    const std::vector<int32_t> row0 = out_row, col0 = out_col; const std::vector<double> val0 = out_val;
    std::vector<unsigned char> done(n, 0);
    MergeState m;
    auto sweep = [&]() { merge_sweep(slab.data(), lay, K, n, done.data(), m, out_row.data(), out_col.data(), out_val.data()); };
    auto untouched = [&](int64_t it, int from) {
        for (int i = from; i < K; ++i) if (out_row[it * K + i] != row0[it * K + i] || out_col[it * K + i] != col0[it * K + i] || out_val[it * K + i] != val0[it * K + i]) return false;
        return true;
    };
    sweep();
    check(m.n_merged == 0 && m.first_open == 0 && !done[0] && !done[1] && !done[2], "merge_nothing_arrived");
    // row 1: `filled` arrives before any slot
    filled[1] = 2; sweep();
    check(m.n_merged == 0 && !done[1] && untouched(1, 0), "merge_filled_before_slots");
    // ... then its slots but one col word, then that word; one val of slot 1 still the all-ones pattern in between
    row[4] = 1; row[5] = 1; col[4] = 40; val[0 + 4] = 0.5; sweep();
    check(m.n_merged == 0 && !done[1] && untouched(1, 0), "merge_col_word_missing");
    col[5] = 41; sweep();
    check(m.n_merged == 0 && !done[1] && untouched(1, 0), "merge_val_still_sentinel");
    val[5] = 0.25; sweep();
    check(m.n_merged == 1 && done[1] && out_row[4] == 1 && out_row[5] == 1 && out_col[4] == 40 && out_col[5] == 41 && out_val[4] == 0.5 &&
          out_val[5] == 0.25 && untouched(1, 2) && m.first_open == 0, "merge_row_complete_prefix_open");
    // row 2: slots arrive before `filled`; then a `filled` outside [0, K]; then the real one
    for (int i = 0; i < K; ++i) { row[8 + i] = 2; col[8 + i] = 80 + i; val[8 + i] = 1.0 + i; }
    sweep();
    check(m.n_merged == 1 && !done[2] && untouched(2, 0), "merge_slots_before_filled");
    filled[2] = K + 1; sweep();
    check(m.n_merged == 1 && !done[2] && untouched(2, 0), "merge_filled_out_of_range");
    filled[2] = K; sweep();
    check(m.n_merged == 2 && done[2] && out_col[11] == 83 && out_val[11] == 4.0 && m.first_open == 0, "merge_full_row");
    // a second sweep merges nothing twice: the caller's slots are rewritten by the caller and must stay
    out_val[4] = 9.0; sweep();
    check(m.n_merged == 2 && out_val[4] == 9.0, "merge_exactly_once");
    out_val[4] = 0.5;
    // row 0: filled = 0 -- nothing copied, the row counts, the prefix closes over all three
    filled[0] = 0; sweep();
    check(m.n_merged == 3 && done[0] && untouched(0, 0) && m.first_open == 3, "merge_empty_row_closes_prefix");
    int64_t first_bad = 0;
    check(verify_merged(slab.data(), lay, K, n, out_row.data(), out_col.data(), out_val.data(), &first_bad) == 0 && first_bad == -1, "verify_clean");
    col[9] = 999;                                          // the slab changes after the merge
    check(verify_merged(slab.data(), lay, K, n, out_row.data(), out_col.data(), out_val.data(), &first_bad) == 1 && first_bad == 2, "verify_reports_changed_row");
    col[9] = 81; filled[1] = -1;
    check(verify_merged(slab.data(), lay, K, n, out_row.data(), out_col.data(), out_val.data(), &first_bad) == 1 && first_bad == 1, "verify_reports_bad_filled");
    filled[1] = 2;
    // scatter_filled: a gathered slab of `per` = 3 rows of which 2 are this call's, written at row0 = 5: only filled > 0 rows
    std::vector<int32_t> big_row(8 * K, -3), big_col(8 * K, -4); std::vector<double> big_val(8 * K, -5.0);
    scatter_filled(slab.data(), n, K, 5, 2, big_row.data(), big_col.data(), big_val.data());
    bool ok = true;
    for (int64_t r = 0; r < 8; ++r) for (int i = 0; i < K; ++i) {
        const bool written = r == 6 && i < 2;              // slab row 1 (filled 2) -> caller row 6; slab row 0 is empty; row 2 is beyond n_rows
        ok &= big_row[r * K + i] == (written ? 1 : -3) && big_col[r * K + i] == (written ? 40 + i : -4) && big_val[r * K + i] == (written ? (i ? 0.25 : 0.5) : -5.0);
    }
    check(ok, "scatter_filled_rows");
}

}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd) || cmd[0] == '#') continue;
        if (cmd == "consts") {
            in >> kc.ctl_bytes >> kc.three_lds >> kc.min_cap >> kc.topk_bins >> kc.bucket_cap >> kc.unit_shift >> kc.sk_max_pushers >> kc.sk_max_coef >> kc.sk_tie;
        } else if (cmd == "handle") {
            h = Handle(); int acsr = 1;
            in >> h.n_nodes >> h.nnz >> h.num_cus >> acsr; h.acsr_ok = acsr != 0;
        } else if (cmd == "opt") {
            std::string k; long long v = 0; in >> k >> v;
            if (!set_option(k, v)) { std::printf("ERROR unknown option %s\n", k.c_str()); return 2; }
        } else if (cmd == "occ") {
            in >> occ_sketch >> occ.general[0] >> occ.general[1] >> occ.general[2] >> occ.general[3];
        } else if (cmd == "call") {
            int n_coef = 0, K = 0; double rmax = 0; long long rows = 0;
            in >> n_coef >> rmax >> K >> rows;
            std::vector<double> coef((size_t)std::max(n_coef, 0));
            for (double& c : coef) in >> c;
            do_call(n_coef, rmax, K, rows, coef);
        } else if (cmd == "ws") {
            int n_coef = 0, n_wg = 0, sk_wg = 0; double rmax = 0; long long rows = 0; unsigned long long budget = 0;
            in >> n_coef >> rmax >> n_wg >> sk_wg >> rows >> budget;
            do_ws(n_coef, rmax, n_wg, sk_wg, rows, (size_t)budget);
        } else if (cmd == "est") {
            std::string k; double v = 0; in >> k >> v;
            if (!set_estimate(k, v)) { std::printf("ERROR unknown estimate field %s\n", k.c_str()); return 2; }
        } else if (cmd == "grow") {
            long long rows = 0; double outgrown = 0, back = 0;
            in >> rows >> outgrown >> back;
            grow_estimate(h.est, h.opt.est_level_edges, rows, outgrown, back);
            print_estimate("grow");
        } else if (cmd == "pick") {
            double rmax = 0; int K = 0; Choice ch{};
            in >> rmax >> K >> ch.ms[0] >> ch.ms[1] >> ch.ms[2];
            Shape cands[3];
            choice_candidates(kc, h.n_nodes, h.nnz, rmax, K, cands);
            for (int c = 0; c < 3; ++c) if (!is_candidate(c, K)) ch.ms[c] = 0.f;       // (never timed)
            pick_choice(threshold_picks_sketch(h.n_nodes, rmax), cands, ch);
            std::printf("pick %d %d %d\n", ch.kernel, ch.block_threads, ch.lds_bytes);
        } else if (cmd == "selftest") {
            test_slabs();
            test_merge();
            std::printf("selftest %d\n", n_fail);
        } else {
            std::printf("ERROR unknown command %s\n", cmd.c_str());
            return 2;
        }
        if (!in && !in.eof()) { std::printf("ERROR bad line: %s\n", line.c_str()); return 2; }
    }
    return 0;
}
