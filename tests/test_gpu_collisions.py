"""GPU tests of what follows a hash-table overflow in both GFPush kernels, on graphs whose keys provably share one home slot
(tests/collision_cases.py; the preconditions are asserted on the CPU by tests/test_host_collision_cases.py).

Every LDS table stops probing after kMaxProbe = 24 slots.  The rows of the adversarial seeds hold 64 targets with home slot 0 at
every capacity, so each recovery path runs on purpose: the one-wave level's undo, the wipe and partition walk of a direct and of
a sketch level, TOP-K's partitioned aggregation, the general kernel's partition refinement.  Rows are compared with the oracle
(tie-aware), the exact work counters must be the oracle's, no row may be handed back -- and gp_stats.diag_sub[8..10] (level
overflows recovered, one-wave undos, TOP-K aggregation overflows) say that the path ran: > 0 with the adversarial seeds, all
zero when only the controls (same row lengths, pairwise distinct homes) run.

Degrees, row lengths and coefficients of the cases are powers of two: every share and every sum is exact in fp64, so the rows
are the same bits whatever the order of the adds, and options that only change the path must not change a bit.

As measured on an MI355X (level, one-wave, TOP-K), adversarial seeds with their controls, the same at 768 and 512 threads:
merged A (6, 2, 2); sk_seed_merge = 0 A (6, 2, 2); solo_levels = 0 A (6, 0, 2), A + B (9, 0, 4); sk_direct_max = 1 A - C
(12, 0, 4); default B, C (6, 1, 2); sk_target = 4096 B, C (6, 1, 4); general kernel A - C (21, 4, 0) on either CSR, (0, 0, 0) on
the HBM table; every control (0, 0, 0).  Before the fallback after a merged level 1 was fixed, the merged run counted three
one-wave undos and lds_levels 9 against 8."""
import numpy as np
import pytest

import collision_cases as cc
from test_gpu_parity import _assert_parity, _oracle, _run_gpu

pytestmark = pytest.mark.gpu

LEVEL, SOLO, TOPK = 0, 1, 2          # positions in _ovf(): diag_sub[8], [9], [10]


def _ovf(st):
    return tuple(st["diag_sub"][8:11])


@pytest.fixture(scope="module")
def cases():
    return cc.cases()


_oracle_cache = {}


def _expected(cases, seeds):
    key = tuple(int(s) for s in seeds)
    if key not in _oracle_cache:
        _oracle_cache[key] = _oracle(cases.indptr, cases.indices, np.asarray(seeds), cc.COEF, cc.RMAX, cc.TOP_K)
    return _oracle_cache[key]


def _check(cases, seeds, options, want_kernel, label):
    """One call against the oracle: rows, exact counters, nothing failed or handed back.  Returns (rows, stats)."""
    got, st = _run_gpu(cases.indptr, cases.indices, seeds, cc.COEF, cc.RMAX, cc.TOP_K, options=options)
    exp, ost = _expected(cases, seeds)
    print(f"[collisions] {label}: level/solo/topk overflows {_ovf(st)} lds_levels {st['lds_levels']} global_levels {st['global_levels']} "
          f"kernel {st['kernel']} x{st['block_threads']} slots {st['lds_slots']} retried {st['retried_rows']} why {st['diag_sub'][1:8]}")
    assert st["kernel"] == want_kernel, (label, st["kernel"])
    _assert_parity(seeds, cc.TOP_K, got, exp, label=label)
    assert (st["pushes"], st["edges"], st["filled"]) == (ost["pushes"], ost["edges"], ost["filled"]), (label, st, ost)
    assert st["failed_rows"] == 0 and st["retried_rows"] == 0, (label, st["failed_rows"], st["retried_rows"], st["diag_sub"][:8])
    return got, st


def _pair(cases, family, which, options, want_kernel, label):
    """The adversarial seeds with their controls, then the controls alone (whose three counters must be zero)."""
    both = np.concatenate([cases.seeds(family, "adv", which), cases.seeds(family, "ctl", which)])
    got, st = _check(cases, both, options, want_kernel, f"{label} {which} adv+ctl")
    _, st_ctl = _check(cases, cases.seeds(family, "ctl", which), options, want_kernel, f"{label} {which} ctl")
    assert _ovf(st_ctl) == (0, 0, 0), (label, _ovf(st_ctl))
    return got, st


def test_mirrored_key_layout_equals_the_device_copy(cases):
    """Word for word: node_pos, the unit bits, the degree saturation and the column words of the special rows and of 1 000 others."""
    from grand_plus_amd import Graph
    g = Graph(cases.indptr, cases.indices, 0)
    acsr, pos, info, bits, sat = g.self_addressed_csr()
    g.close()
    lay = cc.acsr_layout(cases.indptr)
    node_pos, pos_bits, a_sat, key = lay
    assert (bits, sat) == (pos_bits, a_sat)
    assert np.array_equal(pos, node_pos)
    assert len(acsr) == 32 * int(node_pos[-1]) + 1 and acsr[-1] == -1
    rng = np.random.default_rng(3)
    sample = np.concatenate([np.array(sorted(cases.special.values())), rng.choice(cases.n, size=1000, replace=False)])
    deg = np.diff(cases.indptr)
    for v in sample:
        words = cc.acsr_row_words(cases.indptr, cases.indices, lay, int(v))
        lo = 32 * int(node_pos[v])
        assert np.array_equal(acsr[lo:lo + len(words)], words), int(v)
        assert info[node_pos[v]] == v and (len(words) == 32 or info[node_pos[v] + 1] == deg[v])


SK = {"kernel": 2}


@pytest.mark.parametrize("block", [768, 512])
def test_sketch_kernel_level_one_overflows(cases, block):
    """Seed A: level 1 IS the collision set.  Merged into the seed's call (the fallback after wave 0's undo), as a one-wave level
    of phase_sk_level, as a direct stream (one-wave levels off): the same bits in every row, the same number of levels counted."""
    geo = dict(SK, sk_block_threads=block)
    merged, st_m = _pair(cases, "sk", "A", geo, 2, f"sk x{block} merged")
    assert st_m["block_threads"] == block
    assert _ovf(st_m)[SOLO] > 0 and _ovf(st_m)[LEVEL] > 0, _ovf(st_m)
    plain, st_p = _pair(cases, "sk", "A", dict(geo, sk_seed_merge=0), 2, f"sk x{block} sk_seed_merge=0")
    assert _ovf(st_p)[SOLO] > 0 and _ovf(st_p)[LEVEL] > 0, _ovf(st_p)
    stream, st_s = _pair(cases, "sk", "A", dict(geo, solo_levels=0), 2, f"sk x{block} solo_levels=0")
    assert _ovf(st_s)[LEVEL] > 0 and _ovf(st_s)[SOLO] == 0, _ovf(st_s)
    for other, st_o, name in ((plain, st_p, "sk_seed_merge=0"), (stream, st_s, "solo_levels=0")):
        assert np.array_equal(merged[1], other[1]) and np.array_equal(merged[2], other[2]) and st_m["filled"] == st_o["filled"], name
    assert st_m["lds_levels"] == st_p["lds_levels"], (st_m["lds_levels"], st_p["lds_levels"])


@pytest.mark.parametrize("block", [768, 512])
def test_sketch_kernel_direct_stream_overflows_at_level_two(cases, block):
    """solo_levels = 0, seeds A and B: a MODE 1 direct stream overflows (B: with level 1's state behind it), MODE 3 walks the partitions."""
    _, st = _pair(cases, "sk", "AB", dict(SK, sk_block_threads=block, solo_levels=0), 2, f"sk x{block} solo_levels=0")
    assert _ovf(st)[LEVEL] >= 2 and _ovf(st)[SOLO] == 0, _ovf(st)


@pytest.mark.parametrize("block", [768, 512])
def test_sketch_kernel_sketch_level_overflows(cases, block):
    """sk_direct_max = 1: every level is a sketch level.  FILTER tables the candidates from the log, the wipe stops in front of the
    share table behind cap0, which the split partitions read again."""
    _, st = _pair(cases, "sk", "ABC", dict(SK, sk_block_threads=block, sk_direct_max=1), 2, f"sk x{block} sk_direct_max=1")
    assert _ovf(st)[LEVEL] >= 3, _ovf(st)


@pytest.mark.parametrize("block", [768, 512])
@pytest.mark.parametrize("target", [0, 4096])
def test_sketch_kernel_topk_aggregation_overflows(cases, block, target):
    """Seeds B and C: the set's members all reach TOP-K's aggregation table (sk_target = 4096: with nearly every other node of the
    support), which runs in 2, 4, ... partitions, the running list re-inserted."""
    opts = dict(SK, sk_block_threads=block)
    if target:
        opts["sk_target"] = target
    _, st = _pair(cases, "sk", "BC", opts, 2, f"sk x{block} sk_target={target}")
    assert _ovf(st)[TOPK] > 0, _ovf(st)


GK = {"kernel": 1, "block_threads": 512, "lds_bytes": 53248}     # (the shape CAP_MAX of the general kernel's families is worked out for)


@pytest.mark.parametrize("gk_acsr,family", [(1, "ga"), (0, "gp")])
def test_general_kernel_undo_and_partition_refinement(cases, gk_acsr, family):
    """Its own collision family (hash_a of the self-addressed key / of the packed key).  seedrow = 0 makes level 1 of seed A a
    one-wave level like level 2 of seed B: undone, then refined in partitions; the hub of seed C overflows a table of all waves.
    On the HBM table (force_global) nothing can overflow: the same rows, all counters zero."""
    opts = dict(GK, gk_acsr=gk_acsr, seedrow=0)
    got, st = _pair(cases, family, "ABC", opts, 1, f"gk gk_acsr={gk_acsr}")
    assert st["lds_slots"] <= cc.CAP_MAX[family]
    assert _ovf(st)[SOLO] >= 2 and _ovf(st)[LEVEL] >= 3, _ovf(st)
    _, st1 = _pair(cases, family, "B", dict(GK, gk_acsr=gk_acsr), 1, f"gk gk_acsr={gk_acsr} seedrow")
    assert _ovf(st1)[SOLO] > 0 and _ovf(st1)[LEVEL] > 0, _ovf(st1)
    _, st2 = _pair(cases, family, "C", dict(opts, solo_levels=0), 1, f"gk gk_acsr={gk_acsr} solo_levels=0")
    assert _ovf(st2)[LEVEL] > 0 and _ovf(st2)[SOLO] == 0, _ovf(st2)
    both = np.concatenate([cases.seeds(family, "adv"), cases.seeds(family, "ctl")])
    hbm, st_h = _check(cases, both, dict(opts, force_global=1), 1, f"gk gk_acsr={gk_acsr} force_global")
    assert _ovf(st_h) == (0, 0, 0) and st_h["lds_levels"] == 0 and st_h["global_levels"] > 0, (_ovf(st_h), st_h)
    # the same rows (tie-aware: sums of several shares depend on the order of the adds in their last bits)
    _assert_parity(both, cc.TOP_K, hbm, got, next_value=_expected(cases, both)[0].next_value, label="gk LDS tables against the HBM table")
    assert st_h["filled"] == st["filled"]
