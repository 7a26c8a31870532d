"""GPU tests that hold GFPush's push test `r >= rmax * deg` (graph.h:94) at its threshold in every copy of it, on the graphs of
tests/push_boundary_cases.py (audited on the CPU by tests/test_host_push_boundary.py: each case has a node bit-equal to
rmax * deg, one ulp beside it or one edge beyond it, and each is moved by a deliberate mistake).

Every run compares with the oracle: the kernel asked for ran, nothing failed or was handed back, (pushes, edges, filled) are
the oracle's exactly, values within parity.TAU_VAL with no tie row, and -- by node id -- the neighbours of a node that must
push carry the walk's reserve to 1e-15 while the neighbours of its twin that must not push are absent.

Which copy decides, and the options that move a case between them:
  sketch kernel (kernel = 2)   level 1: phase_sk_seed (sk_seed_merge = 1, seed of <= 256 edges), the one-wave level
                               (sk_seed_merge = 0), SCAN behind a direct stream (solo_levels = 0), FILTER + SCAN
                               (sk_direct_max = 1: every level is a sketch level); deeper levels: the one-wave level, SCAN,
                               FILTER + SCAN; both workgroup shapes.  K <= 128 there: seeds run under the largest K at which
                               their K-th and (K+1)-th reserve values differ (Case.cut_groups), so no tie rule is invoked.
  general kernel (kernel = 1)  the seed row (seedrow = 1) or a table drain (seedrow = 0) at level 1; the one-wave level or
                               the dense drain (solo_levels) deeper; the HBM table's drain (force_global); on the packed CSR
                               and, with the graph padded by isolated nodes to 65 536, on the self-addressed one (gk_acsr).
                               K is above every row's support there: every reserve value is compared.
No counter tells a one-wave level from a whole-workgroup one: both settings run and both must equal the oracle."""
import pytest

import push_boundary_cases as pb
from test_gpu_parity import _assert_parity, _oracle, _run_gpu

pytestmark = pytest.mark.gpu

CASES = pb.cases()

# (sk_block_threads, sk_seed_merge, solo_levels, sk_direct_max)
SK_RUNS = [(768, 1, 1, 0), (768, 0, 1, 0), (768, 1, 0, 0), (768, 0, 0, 0), (768, 1, 1, 1), (768, 0, 0, 1),
           (512, 1, 1, 0), (512, 1, 0, 0), (512, 1, 1, 1)]
# (gk_acsr, seedrow, solo_levels, force_global) on the padded graph
GK_RUNS = [(1, 1, 1, 0), (1, 0, 1, 0), (1, 1, 0, 0), (1, 0, 0, 0), (0, 1, 1, 0), (0, 0, 1, 0), (0, 1, 0, 0), (0, 0, 0, 0),
           (0, 1, 1, 1), (0, 0, 0, 1)]

_cache = {}


def _expected(case, pos, K, padded):
    key = (case.name, tuple(pos), K, padded)
    if key not in _cache:
        indptr, indices = case.padded() if padded else (case.indptr, case.indices)
        _cache[key] = _oracle(indptr, indices, case.seeds[pos], case.coef, case.rmax, K)
    return _cache[key]


def _walks(case):
    if ("walk", case.name) not in _cache:
        _cache[("walk", case.name)] = pb.walk_case(case)[0]
    return _cache[("walk", case.name)]


def _run(case, pos, K, options, want_kernel, label, padded=False):
    """One call on the seeds at positions `pos` against the oracle and the walk.  Returns the stats."""
    indptr, indices = case.padded() if padded else (case.indptr, case.indices)
    seeds = case.seeds[pos]
    got, st = _run_gpu(indptr, indices, seeds, case.coef, case.rmax, K, options=options)
    exp, ost = _expected(case, pos, K, padded)
    print(f"[push boundary] {label}: kernel {st['kernel']} x{st['block_threads']} pushes {st['pushes']} / {ost['pushes']} edges {st['edges']} / "
          f"{ost['edges']} filled {st['filled']} / {ost['filled']} lds_levels {st['lds_levels']} global_levels {st['global_levels']} "
          f"degree_lookups {st['degree_lookups']} sketch_candidate_edges {st['sketch_candidate_edges']} {st['kernel_ms']:.2f} ms")
    assert st["kernel"] == want_kernel, (label, st["kernel"])
    assert st["failed_rows"] == 0 and st["retried_rows"] == 0, (label, st["failed_rows"], st["retried_rows"], st["diag_sub"][:8])
    assert (st["pushes"], st["edges"], st["filled"]) == (ost["pushes"], ost["edges"], ost["filled"]), (label, st, ost)
    from grand_plus_amd.parity import TAU_VAL
    rep = _assert_parity(seeds, K, got, exp, next_value=ost["next_value"])
    assert rep.tie_rows == 0 and rep.max_rel_err <= TAU_VAL, (label, rep.tie_rows, rep.max_rel_err)
    # by node id: the neighbours of every threshold node of these seeds
    walks = _walks(case)
    for t in case.targets:
        where = [i for i, p in enumerate(pos) if case.seeds[p] == t.seed]
        if not where or t.node == t.seed and t.level > 0:
            continue
        i = where[0]
        row = {int(c): v for c, v in zip(got[1][i * K:(i + 1) * K], got[2][i * K:(i + 1) * K]) if v > 0.0}
        in_oracle = {int(c) for c, v in zip(exp[1][i * K:(i + 1) * K], exp[2][i * K:(i + 1) * K]) if v > 0.0}
        reserve = walks[pos[i]].reserve
        for v in case.neighbours(t.node):
            if t.pushes:
                assert v in row or v not in in_oracle, (label, t, v)                       # (below the cut of a sketch-kernel K)
                if v in row:
                    assert abs(row[v] - reserve[v]) <= 1e-15 * reserve[v], (label, t, v, row[v], reserve[v])
            else:
                assert v not in row and v not in reserve, (label, t, v)
    return st


@pytest.mark.parametrize("name", pb.GPU_CASES)
def test_sketch_kernel_at_the_threshold(name):
    case = CASES[name]
    for bits in case.degree_bits:
        extra = {} if bits == 31 else {"max_degree_bits": bits}
        for K, pos in sorted(case.cut_groups().items()):
            levels = {}
            for block, merge, solo, dmax in SK_RUNS:
                opts = dict(extra, kernel=2, sk_block_threads=block, sk_seed_merge=merge, solo_levels=solo)
                if dmax:
                    opts["sk_direct_max"] = 1
                st = _run(case, pos, K, opts, 2, f"{name} sk K{K} bits{bits} x{block} merge{merge} solo{solo} dmax{dmax}")
                assert st["block_threads"] == block
                if dmax and _walks_push_past_level_zero(case, pos):
                    assert st["sketch_candidate_edges"] > 0, (name, opts)
                levels[(block, merge, solo, dmax)] = st["lds_levels"]
            # level 1 in the call of level 0 is counted once, as without the merge
            assert levels[(768, 1, 1, 0)] == levels[(768, 0, 1, 0)], levels
            if case.path == "filter":                                 # 256-cell level sketch: collisions may only add candidates
                for block in (768, 512):
                    st = _run(case, pos, K, dict(extra, kernel=2, sk_block_threads=block, sk_direct_max=1, sk_lg_mu=8), 2,
                              f"{name} sk K{K} x{block} dmax1 sk_lg_mu 8")
                    assert st["sketch_candidate_edges"] > 0 or not _walks_push_past_level_zero(case, pos)


def _walks_push_past_level_zero(case, pos):
    """Some row of the call has a level >= 1 with a node that pushes (so a sketch level has a candidate edge)."""
    return any(d.taken and d.level >= 1 for p in pos for d in _walks(case)[p].decisions)


def _gk_runs(case):
    """seedrow decides level 1 alone: the cases that run most calls (three degree widths; 5 000-edge levels in two K groups) and
    hold their targets at level 2 take it off only once, with the HBM table."""
    return [r for r in GK_RUNS if r[1] == 1 or r[3] == 1] if case.path in ("saturation", "wide") else GK_RUNS


@pytest.mark.parametrize("name", pb.GPU_CASES)
def test_general_kernel_at_the_threshold(name):
    case = CASES[name]
    lookups = {}
    for bits in case.degree_bits + ((31,) if case.path == "saturation" else ()):
        extra = {} if bits == 31 else {"max_degree_bits": bits}
        for K, pos in sorted(case.full_groups().items()):
            _run(case, pos, K, dict(extra, kernel=1), 1, f"{name} gk K{K} bits{bits} as built")
            for acsr, seedrow, solo, glob in _gk_runs(case):
                opts = dict(extra, kernel=1, gk_acsr=acsr, seedrow=seedrow, solo_levels=solo, force_global=glob)
                st = _run(case, pos, K, opts, 1, f"{name} gk K{K} bits{bits} padded acsr{acsr} seedrow{seedrow} solo{solo} global{glob}", padded=True)
                if glob:
                    assert st["global_levels"] > 0 and st["lds_levels"] == 0, (name, opts, st["global_levels"], st["lds_levels"])
                elif any(_walks(case)[p].pushes for p in pos):
                    assert st["global_levels"] == 0 and st["lds_levels"] > 0, (name, opts, st["global_levels"], st["lds_levels"])
                lookups[(bits, acsr, seedrow, solo, glob)] = lookups.get((bits, acsr, seedrow, solo, glob), 0) + st["degree_lookups"]
        if case.path == "wide":                                       # a table too small for the level: walked in hash partitions
            small = dict(extra, kernel=1, block_threads=256, lds_bytes=40960)                # (40 KB hold a K of a few hundred at most)
            for K2, pos2 in sorted(case.cut_groups().items()):
                st = _run(case, pos2, K2, small, 1, f"{name} gk K{K2} 256 x 40 KB", padded=True)
                assert st["global_levels"] == 0 and st["lds_slots"] < 5000, (st["global_levels"], st["lds_slots"])
                _run(case, pos2, K2, dict(small, solo_levels=0, seedrow=0), 1, f"{name} gk K{K2} 256 x 40 KB seedrow0 solo0", padded=True)
    if case.path == "saturation":
        # a saturated field passes the cheap half of the test for the `between` targets: they look their degree up, and fail
        for bits in case.degree_bits:
            for run in _gk_runs(case):
                assert lookups[(bits,) + run] > lookups[(31,) + run], (bits, run, lookups[(bits,) + run], lookups[(31,) + run])


def test_saturation_values_of_both_copies():
    """max_degree_bits = 2 / 3 give deg_sat 3 / 7 on the packed CSR (collision_cases.packed_layout mirrors it) and on the
    self-addressed copy, read back through the internal accessor; the case's degrees stand around exactly these values."""
    import collision_cases as cc
    from grand_plus_amd import Graph
    case = CASES["saturation"]
    indptr, indices = case.padded()
    for bits in case.degree_bits:
        g = Graph(indptr, indices, 0)
        g.set_option("max_degree_bits", bits)
        _, _, _, unit_bits, sat = g.self_addressed_csr()
        g.close()
        lay = cc.acsr_layout(indptr, bits)
        assert sat == (1 << bits) - 1 == lay[2] and unit_bits == lay[1]
        assert cc.packed_layout(indptr, bits)[1] == sat
        degs = {int(indptr[t.node + 1] - indptr[t.node]) for t in case.targets}
        assert {sat - 1, sat, sat + 1, 4 * sat} <= degs
