"""CPU audit of tests/select_boundary_cases.py: every case is exact (its sums are order-independent), the float64 walk equals the
oracle, every case holds the tie, distance or edge it claims, the mirror of the select rule equals the strict reference, every
deliberate mistake moves the slot-ordered row of some case and every case is moved by some mistake.  Also records how near the
inputs of the older tests come to a tie at the K-th place.  No GPU, no native library but the oracle."""
import functools
import os

import numpy as np
import pytest

import select_boundary_cases as sb

CASES = sb.cases()


def test_the_gpu_list_is_the_case_list():
    assert tuple(CASES) == sb.GPU_CASES


@pytest.mark.parametrize("name", sb.GPU_CASES)
def test_every_case_is_exact(name):
    """Per node: the per-edge terms (the finest grain either kernel adds at) summed ascending, descending and shuffled give the
    same bits as the walk's reserve; sums of more than two terms are dyadic within one 53-bit window, so every partial sum of
    every grouping is a double too."""
    c = CASES[name]
    assert c.n_nodes <= 1 << 21 and 1 <= len(c.seeds) <= 8
    rng = np.random.default_rng(11)
    for seed, w in zip(c.seeds, c.walks()):
        per_level, per_edge = sb.records(c, seed)
        assert per_edge.keys() == w.reserve.keys() and len(w.reserve) <= 6000
        for node, terms in per_edge.items():
            vals = [v for _, v in terms]
            sums = sb.sums_in_three_orders(vals, rng) + sb.sums_in_three_orders([v for _, v in per_level[node]], rng)
            assert all(sb._bits(s) == sb._bits(w.reserve[node]) for s in sums), (name, node, sums, w.reserve[node])
            assert len(vals) <= 2 or sb.one_window(vals), (name, node, vals)


@pytest.mark.parametrize("name", sb.GPU_CASES)
def test_walk_equals_the_oracle(name):
    """Same values in the same number of slots, bit for bit; same columns except inside the tie group of the K-th value, which the
    oracle's (K+1)-th value proves; next_value as the walk says."""
    from oracle import pyoracle
    c = CASES[name]
    for K in c.ks:
        _, col, val, st = pyoracle.gfpush(c.indptr, c.indices, c.seeds, c.coef, c.rmax, K, want_next=True)
        filled = 0
        for i, w in enumerate(c.walks()):
            exp = sb.select_exact(w.reserve, K)
            got = sorted(((int(k), v) for k, v in zip(col[i * K:(i + 1) * K], val[i * K:(i + 1) * K]) if v > 0.0), key=lambda cv: (-cv[1], cv[0]))
            assert [sb._bits(v) for _, v in got] == [sb._bits(v) for _, v in exp], (name, K, i)
            nxt = sb.next_after_k(w.reserve, K)
            assert sb._bits(st["next_value"][i]) == sb._bits(nxt), (name, K, i, st["next_value"][i], nxt)
            kth = exp[-1][1]
            assert {k for k, v in got if v != kth} == {k for k, v in exp if v != kth}, (name, K, i)
            if {k for k, _ in got} != {k for k, _ in exp}:
                assert nxt == kth, (name, K, i)
            assert all(w.reserve[k] == v for k, v in got)
            filled += len(exp)
        assert filled == st["filled"]


def _sep_bytes(ids):
    """The byte positions in which two of the ids differ."""
    ids = np.asarray(list(ids), np.int64)
    return {b for b in range(4) if len(set(((ids >> (8 * b)) & 255).tolist())) > 1}


def _sep_digits(ids):
    """The general select's id digits (6: bits 12-23 of ~column, 7: bits 0-11) in which two of the ids differ."""
    ids = np.asarray(list(ids), np.int64)
    return {d for d, sh in ((6, 12), (7, 0)) if len(set(((ids >> sh) & 4095).tolist())) > 1}


# which id bytes (sketch select) and radix digits (general select) separate the members, in node ids and in unit numbers alike
TIE_LAYOUT_CLAIMS = {"tie_consec": ({0, 1}, {7}), "tie_step256": ({1, 2}, {6, 7}), "tie_step64k": ({2}, {6}), "tie_straddle4096": ({0, 1}, {6, 7})}


@pytest.mark.parametrize("name", sb.GPU_CASES)
def test_case_holds_what_it_claims(name):
    c = CASES[name]
    cl = c.claims
    walks = c.walks()
    if c.path == "tie":
        K, w = c.ks[0], walks[0]
        group = [n for n, v in w.reserve.items() if sb._bits(v) == sb._bits(cl["group_value"])]
        assert sorted(group) == sorted(cl["group"])
        above = sum(v > cl["group_value"] for v in w.reserve.values())
        assert above == cl["above"] and above < K < above + len(group) and K <= 128
        exp = sb.select_exact(w.reserve, K)
        assert [k for k, _ in exp[above:]] == sorted(group)[:K - above]               # the group's smallest columns, ascending
        others = [k for k, _ in exp[:above]]
        if name.endswith("_low") or name.startswith("tie_g"):
            assert max(group) < min(others)
        if name.endswith("_high"):
            assert min(group) > max(others)
        units = c.units()
        assert all(units[a] < units[b] for a, b in zip(sorted(group), sorted(group)[1:]))
        for prefix, (bytes_, digits) in TIE_LAYOUT_CLAIMS.items():
            if name.startswith(prefix):
                for space in (group, [int(units[g]) for g in group]):
                    assert _sep_bytes(space) == bytes_ and _sep_digits(space) == digits, (name, _sep_bytes(space), _sep_digits(space))
    elif c.path == "near":
        K = c.ks[0]
        for i, w in enumerate(walks):
            exp = sb.select_exact(w.reserve, K + 1)
            (ck, vk), (cn, vn) = exp[K - 1], exp[K]
            assert sb.ulps(vk, vn) == cl["near_ulps"], (name, sb.ulps(vk, vn))
            assert (ck > cn) == (i == 0)                                              # seed 0: the larger value has the larger column
            crowd = [v for v in w.reserve.values() if sb._bits(v) >> 16 == sb._bits(vk) >> 16]
            assert len(crowd) >= 296 > sb.kBucketCap                                 # the general select reaches digit 4 and beyond
            xs = [k for k, v in w.reserve.items() if v == vk]
            ys = [k for k, v in w.reserve.items() if v == vn]
            assert len(xs) == 96 and len(ys) == 200 and ((min(xs) > max(ys)) if i == 0 else (max(xs) < min(ys)))
    elif c.path == "support":
        w = walks[0]
        pos = [k for k, v in w.reserve.items() if v > 0.0]
        assert len(pos) == cl["positives"] and {len(pos) - 1, len(pos), len(pos) + 1} <= set(c.ks) | {0}
        for z in cl.get("zeros", ()):
            assert w.reserve[z] == 0.0 and not np.signbit(w.reserve[z])
        for z in cl.get("negatives", ()):
            assert w.reserve[z] < 0.0
        if "first_tie" in cl:
            top = sb.select_exact(w.reserve, 3)
            assert [k for k, _ in top] == cl["first_tie"] and len({v for _, v in top}) == 1 and 1 in c.ks
    elif c.path == "edge":
        K, w = c.ks[0], walks[0]
        exp = sb.select_exact(w.reserve, K + 1)
        assert exp[K - 1][1] == cl["edge"] == sb._counter_edge(cl["edge"]) and sb.ulps(exp[K - 1][1], exp[K][1]) == 1
        assert sb._counter_edge(exp[K][1]) < cl["edge"]                               # the next counter down (the next binade for m = 0)
    elif c.path == "prune":
        K, w = c.ks[0], walks[0]
        per_level, _ = sb.records(c, c.seeds[0])
        n_levels = len(c.coef)
        by_level = {}
        for recs in per_level.values():
            for lvl, v in recs:
                by_level.setdefault(lvl, []).append(v)
        assert [len(by_level[l]) >= 2 * K for l in sorted(by_level)] == [False, False, True]      # the last level is the threshold level
        seg = sorted(by_level[2], reverse=True)
        assert seg[K - 1] == cl["tau"] == sb._counter_edge(seg[K - 1]) and seg[K - 2] > sb._counter_edge(seg[K - 1], upper=True) > seg[K - 1]
        assert [v for _, v in per_level[cl["X"]]] == [cl["tau"] / n_levels] * n_levels and w.reserve[cl["X"]] == cl["tau"]
        thr = cl["tau"] / n_levels * 0.99999
        assert thr < cl["tau"] / n_levels < thr * 1.00002
        assert thr < w.reserve[cl["Y"]] < cl["tau"] * 0.99999 and all(v < thr for _, v in per_level[cl["Z"]])
        exp = [k for k, _ in sb.select_exact(w.reserve, K)]
        assert exp[-1] == cl["X"] and w.reserve[cl["W"]] == cl["tau"] and cl["W"] > cl["X"]
        assert cl["Y"] not in exp and cl["Z"] not in exp and cl["W"] not in exp
    elif c.path == "heavy":
        K, w = c.ks[0], walks[0]
        per_level, _ = sb.records(c, c.seeds[0])
        by_level = {}
        for recs in per_level.values():
            for lvl, v in recs:
                by_level.setdefault(lvl, []).append(v)
        first = next(l for l in sorted(by_level) if len(by_level[l]) >= 2 * K)
        assert first == cl["thr_level"] < len(c.coef) - 1                             # not the last level: phase_tau takes tau
        seg = sorted(by_level[first], reverse=True)
        assert seg[K - 1] == cl["tau"] == sb._counter_edge(seg[K - 1])
        thr = cl["tau"] / len(c.coef) * 0.99999
        heavy = sum(v >= thr for l in by_level if l > first for v in by_level[l])
        exp = sb.select_exact(w.reserve, K + 1)
        if "heavy_cap" in cl:
            assert heavy == cl["heavy_records"] and (heavy > cl["heavy_cap"]) == name.endswith("overflow") and c.n_nodes + 1 == 65
            group = [k for k, v in w.reserve.items() if v == exp[K - 1][1]]
            above = sum(v > exp[K - 1][1] for v in w.reserve.values())
            assert len(group) == 63 and above == 1 < K < above + len(group)
        else:
            assert heavy > 0 and exp[K - 1][0] == cl["X"] and exp[K][0] == cl["next"] and w.reserve[cl["next"]] >= cl["tau"] * 0.99999
    else:
        raise AssertionError(c.path)


def _mirror_runs(c):
    """(label, kwargs) of every mirror configuration a case is held to."""
    runs = [("general", dict(model="general", coef_nonneg=bool((c.coef >= 0).all())))]
    if 2 in c.kernels:
        units = c.units()
        unit_of = lambda n: int(units[n])                                             # noqa: E731
        runs += [("sketch", dict(model="sketch", unit_of=unit_of)), ("sketch target 3", dict(model="sketch", sk_target=3, unit_of=unit_of)),
                 ("sketch 2 parts", dict(model="sketch", parts=2, unit_of=unit_of))]
    return runs


def _rows(c, mut, label, kw):
    out = []
    for seed in c.seeds:
        per_level, _ = sb.records(c, seed)
        for K in c.ks:
            out.append([(k, sb._bits(v)) for k, v in sb.select_mirror(per_level, K, len(c.coef), mut=mut, **kw)])
    return out


@functools.lru_cache(maxsize=None)
def _exact_rows(name):
    c = CASES[name]
    return [[(k, sb._bits(v)) for k, v in sb.select_exact(w.reserve, K)] for w in c.walks() for K in c.ks]


@pytest.mark.parametrize("name", sb.GPU_CASES)
def test_mirror_equals_the_strict_reference(name):
    c = CASES[name]
    for label, kw in _mirror_runs(c):
        assert _rows(c, None, label, kw) == _exact_rows(name), (name, label)


def test_every_mistake_is_seen_and_every_case_earns_its_place():
    seen_by = {m: [] for m in sb.SELECT_MUTANTS}
    moved = {name: [] for name in sb.GPU_CASES}
    for name in sb.GPU_CASES:
        c = CASES[name]
        exact = _exact_rows(name)
        for m in sb.SELECT_MUTANTS:
            for label, kw in _mirror_runs(c):
                if (m in sb.SKETCH_MUTANTS) > (kw["model"] == "sketch"):
                    continue
                if _rows(c, m, label, kw) != exact:
                    seen_by[m].append(name)
                    moved[name].append(m)
                    break
    for m, hits in seen_by.items():
        print(f"[select boundary] {m}: {len(hits)} case(s): {hits}")
        if m in sb.INDISTINGUISHABLE:
            assert not hits, f"{m} is declared indistinguishable but {hits} see it: take it off the list"
        else:
            assert hits, f"no case sees the mistake {m}"
    assert len(sb.INDISTINGUISHABLE) <= 2 and set(sb.INDISTINGUISHABLE) <= set(sb.SELECT_MUTANTS)
    for name, ms in moved.items():
        print(f"[select boundary] {name}: moved by {sorted(set(ms))}")
        assert ms, f"case {name} is moved by no mistake: it does not belong in GPU_CASES"


# ------------------------------------------------------------------ the gap these cases close, recorded

NEAR_REL = 2.0 ** -40
# (rows, rows whose K-th and (K+1)-th totals are within 2^-40 relative but not equal, rows where they are equal)
NEAR_EXPECTED = {"small mag-ppr": (512, 0, 1), "pubmed ppr": (150, 1, 22)}


def _near_inputs():
    from grand_plus_amd import synth
    from grand_plus_amd.recipes import RECIPES
    indptr, indices = synth.shape_csr("small")
    r = RECIPES[("mag", "ppr")]
    yield "small mag-ppr", indptr, indices, synth.seeds(len(indptr) - 1, 512), r.coef(), r.rmax, r.top_k
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pubmed.npz"))
    yield "pubmed ppr", z["indptr"], z["indices"], z["seeds"][:150], z["ppr_coef"], float(z["ppr_params"][0]), int(z["ppr_params"][1])


def test_the_gap_recorded():
    """How near the K-th and (K+1)-th totals of the older tests' inputs come: what a comparator that forgives 1e-12 could have seen.
    DESIGN.md section 7s states these figures; if a change to synth or to the golden files moves them, update NEAR_EXPECTED and 7s."""
    from oracle import pyoracle
    for label, indptr, indices, seeds, coef, rmax, K in _near_inputs():
        _, _, val, st = pyoracle.gfpush(indptr, indices, seeds, coef, rmax, K, want_next=True)
        v = val.reshape(len(seeds), K)
        full = (v > 0.0).sum(1) == K
        kth = np.where(full, v.min(1, where=v > 0.0, initial=np.inf), 0.0)
        nxt = np.asarray(st["next_value"])
        live = full & (nxt > 0.0)
        equal = int((live & (kth == nxt)).sum())
        near = int((live & (kth != nxt) & (kth - nxt <= NEAR_REL * kth)).sum())
        print(f"[select boundary] gap {label}: {len(seeds)} rows at K = {K}, {int(live.sum())} with a (K+1)-th total, {near} within 2^-40 but "
              f"not equal, {equal} equal")
        assert (len(seeds), near, equal) == NEAR_EXPECTED[label], (f"{label}: {(len(seeds), near, equal)}, recorded {NEAR_EXPECTED[label]}: "
                                                                   "update NEAR_EXPECTED here and the table in DESIGN.md section 7s")
