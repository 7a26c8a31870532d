"""CPU tests of the dense-LDS GFPush kernel's host side (option kernel = 3): the decisions dense_wanted / dense_plan of
grand_plus_amd/csrc/gfpush_plan.hpp through tests/native/gfpush_dense_check.cpp (stand-alone, built with the address and
undefined-behaviour sanitizers), the numpy mirror of tests/dense_cases.py with its deliberate mistakes, and the condition the
GPU test of the golden rows rests on: no push decision of the six citation recipes comes near its threshold."""
import os

import numpy as np
import pytest

import dense_cases as dc
import native_check
import push_boundary_cases as pb

GOLD = os.path.join(os.path.dirname(__file__), "golden")
LDS = 163840
FIELDS = ("fits", "csr_lds", "lds_bytes", "block", "workgroups", "n_pad", "off_hist", "off_cur", "off_next", "off_reserve", "off_marks",
          "off_indptr", "off_indices", "state_end")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = native_check.build(tmp_path_factory, "gfpush_dense_check")
    return lambda lines: native_check.run(exe, list(lines))


@pytest.fixture(scope="module")
def cap(checker):
    max_nodes, lds, ctl, hist = native_check.ints(checker(["consts"]))[0]
    assert lds == LDS and max_nodes >= 5120 and max_nodes == dc.DENSE_MAX_NODES
    # the cap follows from the layout: 24 bytes and one mark bit per node behind the control block and the select's histogram
    assert ctl + hist + 24 * max_nodes + max_nodes // 8 <= LDS < ctl + hist + 24 * (max_nodes + 64) + (max_nodes + 64) // 8
    return max_nodes


def plan(checker, n, nnz, K=32, pad=0, block=0, csr=0, cus=256, per_cu=0, max_wg=0, n_seeds=0):
    out = native_check.ints(checker([f"plan {n} {nnz} {K} {pad} {block} {csr} {cus} {per_cu} {max_wg} {n_seeds}"]))[0]
    return dict(zip(FIELDS, out))


def test_dense_wanted_at_the_cap_for_every_kernel_option(checker, cap):
    for n, inside in ((1, True), (cap, True), (cap + 1, False), (0, False)):
        for kernel in (0, 1, 2, 3):
            got = checker([f"wanted {kernel} {n} {4 * n} 3 1e-4 32 0"])
            assert got == ["1" if inside and kernel == 3 else "0"], (n, kernel, got)


def test_dense_wanted_accepts_the_whole_domain_and_nothing_else(checker, cap):
    ask = lambda n_coef, rmax, K: checker([f"wanted 3 2708 10556 {n_coef} {rmax} {K} 0"])[0]
    assert ask(1, 0.0, 1) == "1" and ask(64, 1e-7, 1024) == "1" and ask(3, 0.5, 32) == "1"
    assert ask(0, 1e-4, 32) == "0" and ask(3, -1e-4, 32) == "0" and ask(3, 1e-4, 0) == "0" and ask(3, 1e-4, 1025) == "0"


def test_lds_pad_eating_the_room_sends_the_call_elsewhere(checker, cap):
    state = plan(checker, 2708, 10556)["state_end"]
    room = LDS - state
    pad_ok, pad_over = room & ~15, (room & ~15) + 16
    assert checker([f"wanted 3 2708 10556 3 1e-4 32 {pad_ok}"]) == ["1"]
    assert checker([f"wanted 3 2708 10556 3 1e-4 32 {pad_over}"]) == ["0"]
    assert plan(checker, 2708, 10556, pad=pad_ok)["fits"] == 1 and plan(checker, 2708, 10556, pad=pad_over)["fits"] == 0
    assert checker([f"wanted 3 {cap} 0 3 1e-4 32 0"]) == ["1"] and checker([f"wanted 3 {cap} 0 3 1e-4 32 4096"]) == ["0"]


@pytest.mark.parametrize("K", [1, 32, 1024])
def test_dense_plan_arrays_are_disjoint_aligned_and_inside(checker, cap, K):
    for n in (1, 4, 63, 64, 65, 2708, 3327, cap):
        nnz = 4 * n
        for csr in (0, 1):
            p = plan(checker, n, nnz, K=K, csr=csr)
            assert p["fits"] == 1 and p["n_pad"] == (n + 63) // 64 * 64 >= n
            spans = [(0, p["off_hist"]), (p["off_hist"], 1024), (p["off_cur"], 8 * p["n_pad"]), (p["off_next"], 8 * p["n_pad"]),
                     (p["off_reserve"], 8 * p["n_pad"]), (p["off_marks"], p["n_pad"] // 8)]
            if p["csr_lds"]:
                spans += [(p["off_indptr"], 4 * (n + 1)), (p["off_indices"], 4 * nnz)]
            for (a, la), (b, lb) in zip(spans, spans[1:]):
                assert a % 8 == 0 and b % 8 == 0 and a + la <= b, (n, csr, spans)
            assert spans[-1][0] + spans[-1][1] <= p["lds_bytes"] <= LDS and p["lds_bytes"] % 16 == 0
            assert p["off_next"] == p["off_cur"] + 8 * p["n_pad"]              # TOP-K's list runs over cur | next ...
            assert 16 * min(K, n) <= 16 * p["n_pad"]                          # ... and min(K, N) entries of 16 bytes fit them
            # LDS is what the plan needs, not the whole CU's
            assert p["lds_bytes"] < p["state_end"] + (4 * (n + 1) + 4 * nnz + 16 if p["csr_lds"] else 0) + 16


def test_the_csr_is_staged_exactly_when_it_fits(checker, cap):
    assert plan(checker, 2708, 10556, csr=0)["csr_lds"] == 0
    for n, nnz in ((2708, 10556), (3327, 9228), (2708, 13264), (3327, 12431)):                   # Cora / Citeseer, without and with self loops
        state = plan(checker, n, nnz)["state_end"]
        csr_bytes = (4 * (n + 1) + 7) // 8 * 8 + (4 * nnz + 7) // 8 * 8
        room = LDS - state - csr_bytes
        assert room >= 0
        assert plan(checker, n, nnz, csr=1)["csr_lds"] == 1
        assert plan(checker, n, nnz, csr=1, pad=room & ~15)["csr_lds"] == 1
        p = plan(checker, n, nnz, csr=1, pad=(room & ~15) + 16)
        assert p["fits"] == 1 and p["csr_lds"] == 0 and p["lds_bytes"] == (state + 15) // 16 * 16
    big = (LDS - plan(checker, cap, 0)["state_end"]) // 4
    assert plan(checker, cap, big + 64, csr=1)["csr_lds"] == 0


def test_block_and_workgroups(checker):
    assert plan(checker, 2708, 10556)["block"] == 512 and plan(checker, 2708, 10556, per_cu=0)["workgroups"] == 0
    for block in (256, 512, 1024):
        assert plan(checker, 2708, 10556, block=block)["block"] == block
    assert plan(checker, 2708, 10556, cus=256, per_cu=2, n_seeds=100000)["workgroups"] == 512
    assert plan(checker, 2708, 10556, cus=256, per_cu=2, n_seeds=96, max_wg=2)["workgroups"] == 2
    assert plan(checker, 2708, 10556, cus=256, per_cu=2, n_seeds=7)["workgroups"] == 7


# ---------------------------------------------------------------- the mirror and its mistakes
AUDITED = sorted({(m, n) for m, n, _ in dc.MOVED_BY.values()} | {("pb", "seed_test"), ("pb", "carry"), ("pb", "l1_dup"), ("sb", "support_negative")})


@pytest.mark.parametrize("module,name", AUDITED)
def test_the_mirror_equals_the_dict_walk(module, name):
    rows, ctr = dc.run_case(module, name)
    exp_rows, exp_ctr = dc.reference_rows(module, name)
    assert ctr == exp_ctr, (ctr, exp_ctr)
    for got, exp in zip(rows, exp_rows):
        assert [c for c, _ in got] == [c for c, _ in exp]
        assert np.allclose([v for _, v in got], [v for _, v in exp], rtol=1e-14, atol=0.0)


@pytest.mark.parametrize("mut", dc.MUTANTS)
def test_every_mistake_moves_a_case(mut):
    module, name, kw = dc.MOVED_BY[mut]
    good = dc.run_case(module, name)
    bad = dc.run_case(module, name, mut=mut, **kw)
    assert bad != good, (mut, module, name)


# ---------------------------------------------------------------- the condition of the golden-row statistics
@pytest.mark.parametrize("name", ["cora", "citeseer"])
@pytest.mark.parametrize("mode", ["ppr", "avg", "single"])
def test_no_push_decision_of_the_golden_recipes_is_near_its_threshold(name, mode):
    """The GPU test asks for the oracle's counters exactly.  Sums into next[] depend on the order of the adds in their last
    bits, so a decision within a few ulps of rmax * deg could fall either way; none of these comes within 2^-40 of it."""
    z = np.load(os.path.join(GOLD, f"{name}.npz"))
    rmax = float(z[f"{mode}_params"][0])
    total, near, _ = pb.near_threshold_counts(z["indptr"], z["indices"], z["seeds"][:256], z[f"{mode}_coef"], rmax, rel=2.0 ** -40)
    print(f"[dense] {name}/{mode}: {total} decisions, {near} within 2^-40 of the threshold")
    assert total > 0 and near == 0
