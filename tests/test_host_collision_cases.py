"""CPU tests of the hash-collision cases (tests/collision_cases.py): the numpy mirror of grand_plus_amd/csrc/gfpush_hash.hpp is held
to the header itself (tests/native/gfpush_hash_check.cpp, built with the address and undefined-behaviour sanitizers), and every
case's precondition -- a set that shares one home slot at every capacity its table can have, a control that shares none -- is
asserted from the mirror alone, against the sets pinned in tests/golden/collision_sets.json.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import collision_cases as cc
import native_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """The path of the check program (test_checker_rejects_what_it_cannot_answer runs it for its exit status)."""
    return native_check.build(tmp_path_factory, "gfpush_hash_check")


def _ask(exe, lines):
    return native_check.ints(native_check.run(exe, lines))


def test_the_hash_header_needs_nothing_but_the_standard_library(tmp_path):
    src = tmp_path / "only_hash.cpp"
    src.write_text('#include "gfpush_hash.hpp"\nint main() { return (int)gp::home_lds(1u, 1024u) + (int)gp::sk_home(1u, 1024u); }\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "grand_plus_amd", "csrc"), str(src)],
                   check=True, timeout=120)
    text = open(os.path.join(ROOT, "grand_plus_amd", "csrc", "gfpush_hash.hpp")).read()
    assert "#include <hip" not in text
    for hdr in ("gfpush_kernels.hpp", "gfpush_sketch.hpp"):                     # ... and the kernel headers keep no second copy
        t = open(os.path.join(ROOT, "grand_plus_amd", "csrc", hdr)).read()
        for fn in ("u32 hash_a(", "u32 hash_b(", "u32 slot_of(", "u32 home_lds(", "u32 sk_home(", "u32 sk_cell(", "kMaxProbe   ="):
            assert fn not in t, (hdr, fn)


def test_python_mirror_equals_the_header(checker):
    assert _ask(checker, ["consts"]) == [[cc.K_MAX_PROBE, cc.K_PROBE_SPAN]]
    rng = np.random.default_rng(1)
    keys = rng.integers(0, 1 << 32, size=10000, dtype=np.uint64)
    keys[:8] = [0, 1, 0xFFFFFF, 0x1000000, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0xFFFFFFFE]
    for cap in (1024, 1172, 2960, 4096):
        for parts in (1, 2, 64):
            got = np.array(_ask(checker, [f"{int(k)} {cap} {parts}" for k in keys]), np.uint64)
            exp = np.stack([cc.hash_a(keys), cc.hash_b(keys), cc.home_lds(keys, cap), cc.sk_home(keys, cap), cc.sk_cell(keys),
                            cc.part_of(keys, parts), cc.slot_of(cc.hash_a(keys), cap)], axis=1)
            assert np.array_equal(got, exp), (cap, parts, np.argwhere(got != exp)[:4])
            assert int(exp[:, 2].max()) < cap - cc.K_PROBE_SPAN and int(exp[:, 3].max()) < cap - cc.K_PROBE_SPAN


def test_checker_rejects_what_it_cannot_answer(checker):
    for bad in ("1 300 1", "1 1024 0", "4294967296 1024 1", "x"):
        r = subprocess.run([checker], input=bad + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (bad, r.returncode, r.stderr)


@pytest.fixture(scope="module")
def cases():
    return cc.cases()


def test_the_search_finds_the_pinned_sets(cases):
    """The sets the search finds are the ones on record: a change of a hash constant, of the layout or of the generator moves them."""
    pin = cc.load_pinned()
    assert pin == cases.pinned()
    assert cc.smallest_n() == cc.N_NODES == pin["n_nodes"]


@pytest.mark.parametrize("family", cc.FAMILIES)
def test_collision_sets_share_one_home_and_controls_share_none(cases, family):
    """From the mirror alone, on the PINNED node ids: >= 50 members with one home slot at each capacity from the one-wave table
    (kMinCap) to the largest table of the family, controls with pairwise distinct homes at every capacity in play."""
    pin = cc.load_pinned()["sets"][family]
    key = cc.family_keys(family, cases.indptr)
    adv, ctl = np.array(pin["adv"]), np.array(pin["ctl"])
    assert len(adv) == cc.SET_SIZE >= 2 * (cc.K_MAX_PROBE + 1) and len(set(adv.tolist())) == len(adv)
    assert len(set(key[adv].tolist())) == len(adv)                              # distinct keys: each claims a slot of its own
    assert int(cc.hash16(family, key[adv]).max()) < cc.window(family)
    for cap in range(cc.K_MIN_CAP, cc.CAP_MAX[family] + 1, 4):
        h = cc.home(family, key[adv], cap)
        assert int(h.min()) == int(h.max()) == 0, (family, cap)
    # one split by hash_b leaves a half that still overflows; the partition walk has to go deeper
    halves = np.bincount(cc.part_of(key[adv], 2).astype(np.int64), minlength=2)
    assert halves.max() > cc.K_MAX_PROBE, halves
    for name, members, caps in (("ctl", ctl, cc.CTL_CAPS[family]), ("hub_ctl", cases.sets[family]["hub_ctl"], cc.HUB_CAPS[family])):
        assert not np.any(np.isin(members, adv))
        for cap in caps:
            h = cc.home(family, key[members], cap)
            assert len(np.unique(h)) == len(members), (family, name, cap)
            assert int(h.min()) >= cc.K_PROBE_SPAN                              # (out of the reach of slot 0's probe sequence)
    fill = np.setdiff1d(cases.sets[family]["hub_adv"], adv)
    assert len(fill) == cc.HUB_LEN - cc.SET_SIZE
    for cap in cc.HUB_CAPS[family]:
        assert len(np.unique(cc.home(family, key[fill], cap))) == len(fill)


def test_csr_is_well_formed_and_special_rows_have_their_lengths(cases):
    indptr, indices, n = cases.indptr, cases.indices, cases.n
    deg = np.diff(indptr)
    assert indptr[0] == 0 and indptr[-1] == len(indices) and deg.min() >= 1                   # no dangling node
    assert indices.min() >= 0 and indices.max() < n
    inner = np.ones(len(indices), bool); inner[indptr[1:-1]] = False
    assert np.all(np.diff(indices.astype(np.int64))[inner[1:]] > 0)                           # strictly increasing inside every row
    special = np.zeros(n, bool); special[list(cases.special.values())] = True
    assert set(np.unique(deg).tolist()) == {1, 2, 4, cc.SET_SIZE, cc.HUB_LEN}                 # powers of two: every share is exact
    plain = np.flatnonzero(~special[:n - 3])                                                  # (the last three rows wrap around)
    assert np.array_equal(indices[indptr[plain]], plain)                                      # a row starts with its self-loop
    for fam in cc.FAMILIES:
        for kind in ("adv", "ctl"):
            a, b, m, c, hub = (cases.special[(fam, kind, r)] for r in cc.ROLES)
            assert deg[a] == deg[m] == cc.SET_SIZE <= cc.K_SK_SOLO_EDGES            # one-wave levels
            assert deg[hub] == cc.HUB_LEN > cc.K_SK_SOLO_EDGES                      # not a one-wave level
            assert deg[b] == 1 and indices[indptr[b]] == m and deg[c] == 1 and indices[indptr[c]] == hub
            mem = cases.members(fam, kind)
            assert np.array_equal(indices[indptr[a]:indptr[a + 1]], np.sort(mem)) and np.array_equal(indices[indptr[m]:indptr[m + 1]], np.sort(mem))
            assert np.all(np.isin(mem, indices[indptr[hub]:indptr[hub + 1]])) or kind == "ctl"
    lay = cc.acsr_layout(indptr)
    assert lay is not None and int(lay[0][-1]) < (1 << 24)                          # (unit numbers fit the 24-bit multiplies)


@pytest.mark.parametrize("family", cc.FAMILIES)
def test_oracle_reaches_every_member(cases, family):
    """The oracle's row of each adversarial seed: every member of the set is reached and pushes (so the kernels must table all
    of them in one level), the row is full, its members are in it and its values are not flat (ties are allowed)."""
    from oracle import pyoracle
    mem = cases.members(family, "adv")
    deg = np.diff(cases.indptr)
    assert np.all(1.0 / cc.HUB_LEN >= cc.RMAX * deg[mem])                           # graph.h:94 holds for every member on every path
    for which, min_frontier, min_pushes in (("A", cc.SET_SIZE, 1 + cc.SET_SIZE), ("B", cc.SET_SIZE, 2 + cc.SET_SIZE), ("C", cc.HUB_LEN, 2 + cc.HUB_LEN)):
        seed = cases.seeds(family, "adv", which)
        row, col, val, st = pyoracle.gfpush(cases.indptr, cases.indices, seed, cc.COEF, cc.RMAX, cc.TOP_K, want_next=True)
        assert st["frontier_max"] >= min_frontier and st["pushes"] >= min_pushes, (which, st)
        assert st["filled"] == cc.TOP_K
        assert len(np.unique(val)) > 1 and np.all(val[:-1] >= val[1:])
        if which != "C":                                                           # (the hub's 320 targets tie: which 32 win is by node id)
            assert np.isin(col, mem).sum() >= cc.TOP_K // 2, (which, col)
        assert st["next_value"][0] > 0.0
