"""CPU tests of GFPush's host-side decisions (grand_plus_amd/csrc/gfpush_plan.hpp): tests/native/gfpush_plan_check.cpp is
built stand-alone with the address and undefined-behaviour sanitizers and run as a child process; each decision goes in as a
line of numbers and comes back as one.  The recorded plans of tests/golden/gfpush_plans.json must come out exactly."""
import os
import subprocess

import pytest

import native_check
import plan_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOC = plan_cases.load()
KC = DOC["kernel_constants"]
CONSTS = "consts " + " ".join(str(KC[k]) for k in ("kCtlBytes", "kThreeLds", "kMinCap", "kTopkBins", "kBucketCap", "kUnitShift",
                                                   "kSkMaxPushers", "kSkMaxCoef", "kSkTie"))
OK, INVALID_ARG, NOMEM = 0, 1, 2
SMALL, TINY = DOC["graphs"]["small"], DOC["graphs"]["tiny"]
CUS = DOC["num_cus"]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """run(lines) -> the program's output lines.  Nothing is preloaded: the sanitizers are linked into the program itself."""
    exe = native_check.build(tmp_path_factory, "gfpush_plan_check")
    return lambda lines: native_check.run(exe, [CONSTS] + list(lines))


def handle(graph, options=None, acsr_ok=1):
    return [f"handle {graph['n_nodes']} {graph['nnz']} {CUS} {acsr_ok}"] + [f"opt {k} {v}" for k, v in (options or {}).items()]


def test_the_header_compiles_alone_with_plain_gxx(tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "gfpush_plan.hpp"\nint main() { return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "grand_plus_amd", "csrc"), str(src)],
                   check=True, timeout=120)
    text = open(os.path.join(ROOT, "grand_plus_amd", "csrc", "gfpush_plan.hpp")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i and "." not in i for i in includes), includes      # the standard library only


# ---------------------------------------------------------------- slab layout, merge, verify, scatter: the program's own cases
SELFTESTS = ["slab_kinds", "layout_general", "layout_sketch", "layout_zero_workgroups", "widen_then_covers", "widen_then_covers_sketch",
             "widen_across_kinds", "widen_empty", "covers_nothing_asked", "packed_layout", "merge_nothing_arrived",
             "merge_filled_before_slots", "merge_col_word_missing", "merge_val_still_sentinel", "merge_row_complete_prefix_open",
             "merge_slots_before_filled", "merge_filled_out_of_range", "merge_full_row", "merge_exactly_once",
             "merge_empty_row_closes_prefix", "verify_clean", "verify_reports_changed_row", "verify_reports_bad_filled",
             "scatter_filled_rows"]


def test_slab_layout_and_merge_rules(checker):
    out = checker(["selftest"])
    assert out == ["PASS " + n for n in SELFTESTS] + ["selftest 0"], out


# ---------------------------------------------------------------- the recorded plans
def occupancy_line(options):
    occ = DOC["occupancy"]
    block, lds = options.get("block_threads", 0), options.get("lds_bytes", 0)
    explicit = occ[f"general_{block or 1024}x{lds or 163840}"] if block or lds else 0
    return f"occ {occ['sketch_768x81920']} {explicit} {occ['general_1024x163840']} {occ['general_768x81920']} {occ['general_512x53248']}"


def call_line(c):
    return f"call {len(c['coef'])} {c['rmax']!r} {c['K']} {c['rows']} " + " ".join(repr(x) for x in c["coef"])


def parse_plan(line):
    f = line.split(" ", 16)
    assert f[0] == "plan", line
    keys = ("status", "kernel", "workgroups", "block_threads", "lds_bytes", "lds_slots", "workspace_bytes", "layout_ok", "realloc", "passes",
            "est_wg", "big_wg", "skl_wg")
    d = {k: int(v) for k, v in zip(keys, f[1:14])}
    d["cur_edges"], d["cur_log"], d["text"] = float(f[14]), float(f[15]), f[16]
    return d


@pytest.mark.parametrize("case", DOC["cases"], ids=[c["id"] for c in DOC["cases"]])
def test_planner_reproduces_the_recorded_plan(checker, case):
    graph = DOC["graphs"][case["graph"]]
    out = checker(handle(graph, case["options"]) + [occupancy_line(case["options"])] + [call_line(c) for c in case["calls"]])
    assert len(out) == len(case["calls"])
    for line, call, want in zip(out, case["calls"], case["expect"]):
        got = parse_plan(line)
        assert got["status"] == OK, line
        assert {k: got[k] for k in plan_cases.PLAN_FIELDS} == {k: want[k] for k in plan_cases.PLAN_FIELDS}, (case["id"], line)
        assert got["layout_ok"] == 1, line                     # arrays disjoint, in order, aligned, inside the bytes the plan reports
        bound = min(graph["nnz"], int(1.001 / call["rmax"]) + 16)
        assert got["cur_edges"] <= bound
        if call is case["calls"][0]:                           # (later calls run on what the earlier ones left: widened, never narrowed)
            assert (got["big_wg"] == 0) == (got["cur_edges"] >= bound and got["cur_log"] == 0.0), line


def test_recorded_cases_are_what_the_issue_lists():
    by = {c["id"]: c for c in DOC["cases"]}
    first = {k: c["expect"][0] for k, c in by.items()}
    assert (first["tiny_defaults"]["block_threads"], first["tiny_defaults"]["workgroups"]) == (512, 3 * CUS)      # three per CU
    assert first["tiny_K200"]["workgroups"] == 2 * CUS and first["tiny_K300"]["workgroups"] == CUS
    assert first["tiny_1_row"]["workgroups"] == 1 and first["tiny_64_rows"]["workgroups"] == 64              # capped by the rows
    assert first["small_K32"]["kernel"] == 2 and first["small_K64"]["kernel"] == 2                             # the threshold pick
    assert first["small_kernel_1"]["kernel"] == 1 and first["small_max_workgroups_3"]["workgroups"] == 3
    assert first["small_workspace_mb_64"]["kernel"] == 1 and first["small_workspace_mb_64"]["workspace_bytes"] <= 64 << 20   # the soft pick dropped
    two = by["small_two_recipes"]["expect"]
    assert two[1]["workspace_bytes"] > two[0]["workspace_bytes"] and two[2]["workspace_bytes"] == two[3]["workspace_bytes"] == two[1]["workspace_bytes"]
    for c in DOC["cases"]:                                      # at the default budget other allocations on the device cannot change the plan
        if "workspace_mb" not in c["options"]:
            assert max(e["workspace_bytes"] for e in c["expect"]) < 4 << 30, c["id"]
        assert all(e["failed_rows"] == 0 for e in c["expect"])


def test_two_recipes_widen_once(checker):
    case = next(c for c in DOC["cases"] if c["id"] == "small_two_recipes")
    out = [parse_plan(x) for x in checker(handle(SMALL) + [occupancy_line({})] + [call_line(c) for c in case["calls"]])]
    assert [p["realloc"] for p in out] == [1, 1, 0, 0]


def test_workspace_mb_64_shrinks_the_slabs_and_drops_the_soft_sketch_pick(checker):
    case = next(c for c in DOC["cases"] if c["id"] == "small_workspace_mb_64")
    p = parse_plan(checker(handle(SMALL, case["options"]) + [occupancy_line({})] + [call_line(case["calls"][0])])[0])
    assert p["kernel"] == 1 and p["skl_wg"] == 0 and p["passes"] == 3           # three per CU -> two -> one
    assert p["cur_edges"] <= 4096.0 < p["cur_edges"] / 0.75                      # shrunk as far as the rule goes
    # ... and where option kernel = 2 insists, the same budget is an error, not a silent general kernel
    q = parse_plan(checker(handle(SMALL, dict(case["options"], kernel=2)) + [occupancy_line({})] + [call_line(case["calls"][0])])[0])
    assert q["status"] == NOMEM and "workspace_mb too small for the sketch kernel's slabs" in q["text"]


# ---------------------------------------------------------------- workspace policy, from the rules its comments state
def ws(checker, pre, n_coef, rmax, n_wg, sk_wg, rows, budget):
    """pre + one plan_workspace -> the fields of its output line."""
    line = checker(pre + [f"ws {n_coef} {rmax!r} {n_wg} {sk_wg} {rows} {budget}"])[-1]
    f = line.split(" ", 16)
    assert f[0] == "ws", line
    keys = ("status", "est_wg", "big_wg", "skl_wg", "fits", "total", "est_per_wg", "big_per_wg", "skl_per_wg", "layout_ok")
    d = {k: int(v) for k, v in zip(keys, f[1:11])}
    d["cur_edges"], d["cur_log"], d["bound"] = float(f[11]), float(f[12]), float(f[13])
    d["recipe_changed"], d["bound_per_wg"], d["text"] = int(f[14]), int(f[15]), f[16]
    return d


HUGE = 1 << 46


def steps_of_075(start, value):
    e, k = start, 0
    while e > value and k < 200:
        e *= 0.75
        k += 1
    return k if e == value else None


def test_slabs_shrink_by_three_quarters_while_they_exceed_half_the_budget(checker):
    pre = handle(SMALL)
    free = ws(checker, pre, 11, 1e-5, 768, 0, 4096, HUGE)
    assert free["status"] == OK and free["cur_edges"] == 32768.0 and free["est_wg"] == 768       # max(32 Ki, bound / 4), nothing to shrink
    need = free["est_per_wg"] * 768
    prev_k = 0
    for budget in (2 * need, 2 * need - 2, need, need // 2):
        d = ws(checker, pre, 11, 1e-5, 768, 0, 4096, budget)
        k = steps_of_075(32768.0, d["cur_edges"])
        assert d["status"] == OK and k is not None and k >= prev_k, (budget, d)
        assert (k == 0) == (budget >= 2 * need)
        assert d["est_wg"] == 768 and d["est_per_wg"] * 768 <= budget // 2 and d["cur_edges"] > 4096.0 * 0.75, d    # the launch is not cut
        assert d["layout_ok"] == 1
        prev_k = k
    assert prev_k >= 2


def test_below_4096_edges_the_launch_is_cut_never_below_one_and_the_sketch_kernel_refuses(checker):
    pre = handle(SMALL)
    for budget in (64 << 20, 1 << 20, 4096):
        d = ws(checker, pre, 11, 1e-5, 768, 0, 4096, budget)
        assert d["status"] == OK and d["cur_edges"] <= 4096.0 < d["cur_edges"] / 0.75, d         # the shrinking stopped at 4096 edges
        assert d["est_wg"] == max(1, budget // 2 // d["est_per_wg"]) and 1 <= d["est_wg"] < 768, d
        assert d["big_wg"] <= d["est_wg"]
        s = ws(checker, pre, 11, 1e-5, 128, 512, 4096, budget)
        assert s["status"] == NOMEM and s["text"].endswith("|workspace_mb too small for the sketch kernel's slabs"), s


def test_big_gets_at_most_eight_workgroups_and_at_most_the_launch(checker):
    pre = handle(SMALL)
    for n_wg, want in ((768, 8), (8, 8), (3, 3), (1, 1)):
        d = ws(checker, pre, 11, 1e-5, n_wg, 0, 4096, HUGE)
        assert (d["est_wg"], d["big_wg"]) == (n_wg, want), d
        assert d["big_per_wg"] == d["bound_per_wg"]
    # ... and as many as what the estimate-sized slabs leave of the budget holds
    free = ws(checker, pre, 11, 1e-5, 20, 0, 4096, HUGE)
    budget = 2 * 20 * free["est_per_wg"]                       # half for the estimate-sized slabs: the other half is what is left
    d = ws(checker, pre, 11, 1e-5, 20, 0, 4096, budget)
    fit = (budget - 20 * free["est_per_wg"]) // free["bound_per_wg"]
    assert 1 <= fit < 8 and d["cur_edges"] == free["cur_edges"] and (d["est_wg"], d["big_wg"]) == (20, fit), d


def test_when_no_bound_sized_slab_fits_big_gets_one_slab_of_what_is_left(checker):
    pre = handle(SMALL)
    free = ws(checker, pre, 11, 1e-7, 1, 0, 4096, HUGE)
    e, w = free["est_per_wg"], free["bound_per_wg"]
    assert free["big_wg"] == 1 and free["cur_edges"] < free["bound"] and e + 16 < w
    budget = 2 * e + 16                                        # half of it holds the estimate-sized slab, the rest is less than a bound-sized one
    d = ws(checker, pre, 11, 1e-7, 1, 0, 4096, budget)
    assert d["status"] == OK and d["est_per_wg"] == e and d["cur_edges"] == free["cur_edges"], d
    assert d["big_wg"] == 1 and d["big_per_wg"] < w and d["big_per_wg"] <= budget - e and d["big_per_wg"] >= d["est_per_wg"], d
    assert d["layout_ok"] == 1


def test_the_estimate_never_exceeds_the_bound_and_at_the_bound_there_is_no_big(checker):
    for options in ({}, {"est_level_edges": 1 << 40}):
        d = ws(checker, handle(TINY, options), 5, 1e-4, 768, 0, 4096, HUGE)
        assert d["bound"] == min(TINY["nnz"], int(1.001 / 1e-4) + 16)
        assert d["cur_edges"] == d["bound"] and d["cur_log"] == 0.0 and d["big_wg"] == 0, d
    d = ws(checker, handle(SMALL, {"est_level_edges": 4096}), 11, 1e-5, 768, 0, 4096, HUGE)
    assert d["cur_edges"] == 4096.0 < d["bound"] and d["cur_log"] == 4 * 4096.0 and d["big_wg"] == 8


def test_a_recipe_change_resets_the_running_estimate_and_flags_the_device_maxima(checker):
    a, b = "ws 11 1e-05 768 0 4096 %d" % HUGE, "ws 5 0.0001 768 0 4096 %d" % HUGE
    grown = ["est recipe_changed 0", "est edges 60000", "est log 500000"]
    out = checker(handle(SMALL) + [a] + grown + [a, b, a, "est recipe_changed 0", "ws 11 1e-05 128 512 4096 %d" % HUGE])

    def f(line):
        x = line.split(" ", 16)
        return float(x[11]), float(x[12]), int(x[14])
    assert f(out[0]) == (32768.0, 131072.0, 1)                # a fresh handle: the first call is a new recipe
    assert f(out[1]) == (60000.0, 500000.0, 0)                # the same recipe keeps what it has learnt
    assert f(out[2])[2] == 1                                  # another recipe ...
    assert f(out[3]) == (32768.0, 131072.0, 1)                # ... and back: the estimate starts over, the flag is set again
    assert f(out[4])[2] == 1                                  # the other kernel (its log counts edges) is a new recipe too


# ---------------------------------------------------------------- estimate growth
def grow_fields(line):
    f = line.split()
    assert f[0] == "grow", line
    return dict(edges=float(f[1]), log=float(f[2]), grown=int(f[6]), sk_off=int(f[7]), off_rmax=float(f[8]), off_n_coef=int(f[9]))


def test_estimate_growth_follows_the_retry_rate(checker):
    start = ["est rmax 1e-05", "est n_coef 11", "est cur_edges 1000", "est cur_log 4000", "est last_kind 1", "est last_call_rows 10000"]
    again = "est grown_for_call 0"
    out = [grow_fields(x) for x in checker(handle(SMALL) + start + [
        "grow 10000 10 10",                    # 0: the handle starts as "grown": no call has been enqueued
        again, "grow 10000 10 10",             # 1: 0.1 % exactly: nothing, but the call has been looked at
        "grow 10000 5000 5000",                # 2: ... once per call
        again, "grow 10000 11 11",             # 3: above 0.1 %: x 1.5, the log too
        again, "grow 10000 200 200",           # 4: 2 % exactly: still x 1.5 (no change: it is a maximum)
        again, "grow 10000 201 201",           # 5: above 2 %: x 2
        again, "grow 0 201 201",               # 6: a call of no rows: nothing
        "est cur_log 0", "grow 10000 5000 5000",  # 7: the log estimate is not in use: only the edges could grow (2 x 1000: no change)
    ])]
    assert [(o["edges"], o["log"], o["grown"]) for o in out] == [
        (0.0, 0.0, 1), (0.0, 0.0, 1), (0.0, 0.0, 1), (1500.0, 6000.0, 1), (1500.0, 6000.0, 1), (2000.0, 6000.0, 1), (2000.0, 6000.0, 0),
        (2000.0, 6000.0, 1)]
    assert not any(o["sk_off"] for o in out)
    # never when est_level_edges is set
    fixed = [grow_fields(x) for x in checker(handle(SMALL, {"est_level_edges": 4096}) + start + [again, "grow 10000 5000 5000"])]
    assert (fixed[0]["edges"], fixed[0]["log"], fixed[0]["grown"]) == (0.0, 0.0, 0)


def test_the_sketch_kernel_is_switched_off_for_a_recipe_that_keeps_handing_rows_back(checker):
    start = ["est rmax 1e-05", "est n_coef 11", "est cur_edges 1000", "est cur_log 4000", "est last_kind 2", "est last_call_rows 10000"]
    again = "est grown_for_call 0"
    out = [grow_fields(x) for x in checker(handle(SMALL) + start + [
        "est last_sk_soft 1", again, "grow 10000 0 500",        # 5 % exactly: stays on
        again, "grow 10000 300 800",                            # 5 % for other reasons than slab size: stays on
        "est last_sk_soft 0", again, "grow 10000 0 9000",       # option kernel = 2 insisted: never
        "est last_sk_soft 1", "est last_kind 1", again, "grow 10000 0 9000",   # the general kernel ran the call
        "est last_kind 2", again, "grow 10000 0 501",           # a soft pick, above 5 %: off for (rmax, n_coef)
    ])]
    assert [o["sk_off"] for o in out] == [0, 0, 0, 0, 1]
    assert (out[-1]["off_rmax"], out[-1]["off_n_coef"]) == (1e-5, 11)
    # the memory is per recipe: the same call is planned on the general kernel, another recipe still takes the sketch kernel
    coef = " ".join(["0.1"] * 10)
    lines = handle(SMALL) + [occupancy_line({})] + [x.replace("n_coef 11", "n_coef 10") for x in start] + [
        "est last_sk_soft 1", "est grown_for_call 0", "grow 10000 0 501", f"call 10 1e-05 32 4096 {coef}", f"call 10 2e-05 32 4096 {coef}"]
    plans = [parse_plan(x) for x in checker(lines)[1:]]
    assert [p["kernel"] for p in plans] == [1, 2]
    insisted = handle(SMALL, {"kernel": 2}) + lines[1:]
    assert [parse_plan(x)["kernel"] for x in checker(insisted)[1:]] == [2, 2]


# ---------------------------------------------------------------- the measured choice
def pick(checker, graph, rmax, K, ms):
    f = checker(handle(graph) + [f"pick {rmax!r} {K} {ms[0]} {ms[1]} {ms[2]}"])[-1].split()
    assert f[0] == "pick"
    return tuple(int(x) for x in f[1:])


def test_the_threshold_pick_stays_unless_another_candidate_is_more_than_five_per_cent_faster(checker):
    GENERAL, SKETCH, ONE_PER_CU, TWO_PER_CU = (1, 0, 0), (2, 0, 0), (1, 1024, 163840), (1, 768, 81920)
    # small graph, rmax 1e-5: the thresholds pick the sketch kernel; the other shape of the general kernel is one workgroup per CU
    assert pick(checker, SMALL, 1e-5, 32, (9.6, 10.0, 9.6)) == SKETCH
    assert pick(checker, SMALL, 1e-5, 32, (9.0, 10.0, 9.6)) == GENERAL
    assert pick(checker, SMALL, 1e-5, 32, (9.0, 10.0, 8.0)) == ONE_PER_CU
    assert pick(checker, SMALL, 1e-5, 32, (9.0, 10.0, 8.8)) == GENERAL               # 8.8 is not 5 % faster than the pick it would replace (9.0)
    # a candidate timed at 0 is not a candidate
    assert pick(checker, SMALL, 1e-5, 32, (10.0, 0.0, 0.0)) == GENERAL
    assert pick(checker, SMALL, 1e-5, 32, (0.0, 10.0, 0.0)) == SKETCH
    assert pick(checker, SMALL, 1e-5, 32, (0.0, 0.0, 7.0)) == ONE_PER_CU
    assert pick(checker, SMALL, 1e-5, 32, (10.0, 0.0, 5.0)) == ONE_PER_CU
    assert pick(checker, SMALL, 1e-5, 32, (0.0, 0.0, 0.0)) == (0, 0, 0)              # nothing could be timed: the thresholds decide
    # rmax 1e-6: the thresholds pick the general kernel at one workgroup per CU; the other shape is two per CU
    assert pick(checker, SMALL, 1e-6, 32, (10.0, 9.6, 9.6)) == GENERAL
    assert pick(checker, SMALL, 1e-6, 32, (10.0, 9.0, 9.6)) == SKETCH
    assert pick(checker, SMALL, 1e-6, 32, (10.0, 0.0, 9.0)) == TWO_PER_CU
    # K > 256 has no third candidate
    assert pick(checker, SMALL, 1e-5, 300, (10.0, 0.0, 1.0)) == GENERAL
    assert pick(checker, SMALL, 1e-5, 256, (10.0, 0.0, 1.0)) == ONE_PER_CU
