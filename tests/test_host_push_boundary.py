"""CPU audit of tests/push_boundary_cases.py: the float64 walk equals the oracle, every case holds the threshold decision its
name claims, every deliberate mistake moves a counter the GPU file holds exactly, every case is moved by some mistake, and
the shipped sketch filter keeps every true pusher while each of its mistakes drops one.  Also records how near the inputs
of the older tests come to the threshold.  No GPU, no native library but the oracle."""
import os

import numpy as np
import pytest

import push_boundary_cases as pb

CASES = pb.cases()


def test_the_gpu_list_is_the_case_list():
    assert tuple(CASES) == pb.GPU_CASES


@pytest.mark.parametrize("name", pb.GPU_CASES)
def test_walk_equals_the_oracle(name):
    from oracle import pyoracle
    c = CASES[name]
    K = c.full_k()
    _, col, val, st = pyoracle.gfpush(c.indptr, c.indices, c.seeds, c.coef, c.rmax, K)
    walks, pushes, edges = pb.walk_case(c)
    assert (pushes, edges) == (st["pushes"], st["edges"])
    assert sum(w.dangling for w in walks) == st["dangling"] and sum(w.frontier_sum for w in walks) == st["frontier_sum"]
    filled = 0
    for i, w in enumerate(walks):
        got = {int(k): v for k, v in zip(col[i * K:(i + 1) * K], val[i * K:(i + 1) * K]) if v > 0.0}
        exp = {k: v for k, v in w.reserve.items() if v > 0.0}
        assert got.keys() == exp.keys()
        assert all(abs(got[k] - exp[k]) <= 1e-15 * exp[k] for k in exp)
        filled += len(exp)
    assert filled == st["filled"]


_REL_ULPS = {"eq": lambda u: u == 0, "above": lambda u: u >= 1, "below": lambda u: u == -1, "plus1": lambda u: u < -1,
             "between": lambda u: u < -1, "below_far": lambda u: u < -1}


@pytest.mark.parametrize("name", pb.GPU_CASES)
def test_case_preconditions(name):
    """The decision the case is named for: at its level, on a node with the claimed number of in-edges from the level before,
    at the claimed distance from rmax * deg."""
    c = CASES[name]
    assert c.n_nodes <= 11000 and len(c.seeds) <= 16
    walks, _, _ = pb.walk_case(c)
    at_threshold = 0
    for t in c.targets:
        w = walks[c.seeds.tolist().index(t.seed)]
        ds = [d for d in w.decisions if d.node == t.node and d.level == t.level]
        assert len(ds) == 1, (name, t)
        d = ds[0]
        u = pb.ulps(d.r, d.thr)
        assert _REL_ULPS[t.relation](u) and d.taken == t.pushes, (name, t, u, d)
        at_threshold += abs(u) <= 1
        if t.level > 0:
            pushers = {p.node for p in w.decisions if p.level == t.level - 1 and p.taken}
            n_in = sum(c.neighbours(p).count(t.node) for p in pushers) + sum(1 for (l, _, _) in w.returns if l == t.level - 1 and t.node == t.seed)
            assert n_in == t.n_in, (name, t, n_in)
        if t.relation == "between":                                   # cheap half passes (on equality), exact half fails
            sat = next(s for s in (3, 7) if d.deg in (s + 1, 4 * s) and d.r == c.rmax * s)
            assert d.r >= c.rmax * sat and d.r < d.thr
    if name == "many_floor":                                          # held 2^-30 above, not bit-equal (see the case)
        d = [d for d in walks[0].decisions if d.node == c.targets[0].node][0]
        assert 0 < d.r / d.thr - 1 < 2.0 ** -29
    elif name != "carry":
        assert at_threshold >= 1, name
    if name == "dangling":
        (lvl, node, r), = walks[0].returns[:1]
        assert node == c.dangling_node and pb.ulps(r, c.rmax) == -1 and lvl == 3
        seed_d = [d for d in walks[0].decisions if d.node == c.seeds[0] and d.level == 4][0]
        assert seed_d.taken and seed_d.r - r < seed_d.thr <= seed_d.r
    if name == "saturation":
        for hold, (d0, d1) in pb.SAT_CHAINS.items():
            assert (1.0 / d0) / d1 == c.rmax * hold and d0 * d1 * hold == pb.SAT_N
    if name == "seed_test":
        assert len(walks[1].reserve) == 1 and walks[1].pushes == 0


@pytest.mark.parametrize("name", ["many_sum", "many_floor"])
def test_sums_of_many_contributions(name):
    """many_sum: partial sums are exact, so any order of the adds gives the same bits.  many_floor: 64 equal addends; whatever
    the order and grouping, the sum stays within a few ulps -- 2^22 times nearer than the 2^-30 the node is held above at."""
    c = CASES[name]
    w = pb.walk_case(c)[0][0]
    t = c.targets[0]
    shares = []
    for p in w.decisions:
        if p.level == t.level - 1 and p.taken:
            shares += [p.r / p.deg] * c.neighbours(p.node).count(t.node)
    assert len(shares) == 64
    d = [d for d in w.decisions if d.node == t.node][0]
    rng = np.random.default_rng(5)
    for _ in range(20):
        order = rng.permutation(64)
        acc = 0.0
        for i in order:
            acc += shares[i]
        pair = [shares[i] + shares[j] for i, j in zip(order[::2], order[1::2])]          # grouped, as a wave-level reduction would
        while len(pair) > 1:
            pair = [a + b for a, b in zip(pair[::2], pair[1::2])]
        if name == "many_sum":
            assert acc == d.r == pair[0] == d.thr
        else:
            assert abs(acc - d.r) <= 8 * np.spacing(d.r) and abs(pair[0] - d.r) <= 8 * np.spacing(d.r)
            assert min(acc, pair[0]) >= d.thr


def _sat_values(case):
    return [0 if bits == 31 else (1 << bits) - 1 for bits in case.degree_bits]


def test_every_mistake_is_seen_and_every_case_earns_its_place():
    """(pushes, edges) are what the GPU file holds exactly.  Every mistake of the walk moves them on some case; every mistake
    of the filter drops a true pusher of some case; every case of GPU_CASES is moved by at least one of either list."""
    seen_by = {m: [] for m in pb.MUTANTS + pb.FILTER_MUTANTS}
    moved = {name: [] for name in pb.GPU_CASES}
    for name in pb.GPU_CASES:
        c = CASES[name]
        for sat in _sat_values(c):
            _, p0, e0 = pb.walk_case(c)
            for m in pb.MUTANTS:
                _, p1, e1 = pb.walk_case(c, m, sat)
                if (p1, e1) != (p0, e0):
                    seen_by[m].append((name, sat, p1 - p0, e1 - e0))
                    moved[name].append(m)
        for m in pb.FILTER_MUTANTS:
            dropped = sum(1 for s in c.seeds for (_, _, true, cand) in pb.filter_candidates(c, s, m) if true and not cand)
            if dropped:
                seen_by[m].append((name, 0, -dropped, 0))
                moved[name].append(m)
    for m, hits in seen_by.items():
        first = hits[0] if hits else None
        print(f"[push boundary] {m}: {len(hits)} case(s); first {first and first[0]}"
              + (f" (deg_sat {first[1]})" if first and first[1] else "")
              + (f": pushes {first[2]:+d}, edges {first[3]:+d}" if first and m in pb.MUTANTS else f": {first and -first[2]} true pusher(s) dropped"))
        assert hits, f"no case sees the mistake {m}"
    for name, ms in moved.items():
        print(f"[push boundary] {name}: moved by {sorted(set(ms))}")
        assert ms, f"case {name} is moved by no mistake: it does not belong in GPU_CASES"


@pytest.mark.parametrize("name", pb.GPU_CASES)
def test_shipped_filter_keeps_every_true_pusher(name):
    """On cells of their own, and on the hashed cells of the default sketches (2^13, 2^12) and of sk_lg_mu = 8, where
    collisions may only ADD candidates."""
    c = CASES[name]
    for s in c.seeds:
        own = pb.filter_candidates(c, s)
        assert all(cand for (_, _, true, cand) in own if true), name
        for lg in (13, 12, 8):
            hashed = pb.filter_candidates(c, s, lg_mu=lg)
            assert all(h[3] or not o[3] for o, h in zip(own, hashed)), (name, lg)


def test_filter_threshold_is_below_the_product():
    for rmax in sorted({c.rmax for c in CASES.values()}):
        t = float(pb.filter_threshold(rmax))
        assert t <= rmax * 2147483648.0 * (1 - 2.0 ** -10) < float(np.nextafter(np.float32(t), np.float32(np.inf)))


# ------------------------------------------------------------------ the gap these cases close, recorded

GAP_ROWS, PUBMED_ROWS = 64, 150
# (decisions walked, within 2^-20 of rmax * deg, bit-equal to it)
GAP_EXPECTED = {"small mag-ppr": (0, 0), "small reddit-avg": (0, 0), "pubmed ppr": (5, 4), "pubmed avg": (1, 1), "pubmed single": (0, 0)}


def _gap_inputs():
    from grand_plus_amd import synth
    from grand_plus_amd.recipes import RECIPES
    indptr, indices = synth.shape_csr("small")
    seeds = synth.seeds(len(indptr) - 1, GAP_ROWS)
    for key in (("mag", "ppr"), ("reddit", "avg")):
        r = RECIPES[key]
        yield f"small {key[0]}-{key[1]}", indptr, indices, seeds, r.coef(), r.rmax
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pubmed.npz"))
    for mode in ("ppr", "avg", "single"):
        yield f"pubmed {mode}", z["indptr"], z["indices"], z["seeds"][:PUBMED_ROWS], z[f"{mode}_coef"], float(z[f"{mode}_params"][0])


def test_the_gap_recorded():
    """How many push decisions of the inputs the older tests draw lie within 2^-20 of the threshold: none on the graph nearly
    every sketch-kernel test uses, five (four of them bit-equal) on Pubmed-ppr, which reaches the general kernel only.  DESIGN.md
    section 7r states these figures; if a change to synth or to the golden files moves them, update GAP_EXPECTED and 7r."""
    for label, indptr, indices, seeds, coef, rmax in _gap_inputs():
        got = pb.near_threshold_counts(indptr, indices, seeds, coef, rmax)
        print(f"[push boundary] gap {label}: {len(seeds)} rows, {got[0]} decisions, {got[1]} within 2^-20, {got[2]} bit-equal")
        assert got[1:] == GAP_EXPECTED[label], (f"{label}: {got[1:]} decisions near / on the threshold, recorded {GAP_EXPECTED[label]}: "
                                                "update GAP_EXPECTED here and the table in DESIGN.md section 7r")


def test_numpy_walk_counts_what_the_dict_walk_counts():
    """near_threshold_counts against push_walk64's decision list on the cases (exact sums or single contributions there)."""
    for name in ("l2_below", "dangling", "many_sum", "saturation"):
        c = CASES[name]
        walks, _, _ = pb.walk_case(c)
        dec = [d for w in walks for d in w.decisions]
        exp = (len(dec), sum(abs(d.r - d.thr) <= 2.0 ** -20 * d.thr for d in dec), sum(d.r == d.thr for d in dec))
        assert pb.near_threshold_counts(c.indptr, c.indices, c.seeds, c.coef, c.rmax) == exp, name
