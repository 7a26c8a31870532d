"""GPU tests of the dense-LDS GFPush kernel (option kernel = 3, grand_plus_amd/csrc/gfpush_dense.hpp): a row's whole state in
one workgroup's LDS, for graphs of up to dense_cases.DENSE_MAX_NODES nodes.

Every run asserts that the dense kernel ran (st["kernel"] == 3) and that nothing failed or was retried, unless the test is
about a call it must NOT take.  The references are the ones the other kernels are held to: the CPU oracle with its (K+1)-th
value (every tie proven), the golden rows of the real reference, the threshold cases of tests/push_boundary_cases.py with the
assertions of test_gpu_push_boundary._run, and the select cases of tests/select_boundary_cases.py held strictly -- the same
column in the same slot, the value bit-equal, fill untouched from `filled` on.  The dense kernel's statistics are always exact,
so (pushes, edges, filled, support, frontier) are compared with the oracle's wherever no decision sits near its threshold."""
import os

import numpy as np
import pytest

import push_boundary_cases as pb
import select_boundary_cases as sb
from dense_cases import DENSE_MAX_NODES as CAP
from test_gpu_parity import KAT_COEF, KAT_INDICES, KAT_INDPTR, _assert_parity, _oracle, _run_gpu
from test_gpu_push_boundary import _run as _run_push
from test_gpu_select_boundary import FILL, _hold

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
PB_CASES = pb.cases()
SB_CASES = sb.cases()
_cache = {}


def _ran_dense(st, label=""):
    assert st["kernel"] == 3, (label, st["kernel"])
    assert st["failed_rows"] == 0 and st["retried_rows"] == 0, (label, st["failed_rows"], st["retried_rows"])
    assert st["global_levels"] == 0 and st["degree_lookups"] == 0 and st["sketch_candidate_edges"] == 0, label


def _exact_counters(st, ost, label=""):
    got = (st["pushes"], st["edges"], st["filled"], st["support"], st["frontier"])
    exp = (ost["pushes"], ost["edges"], ost["filled"], ost["support_sum"], ost["frontier_sum"])
    assert got == exp, (label, got, exp)


def _against_oracle(indptr, indices, seeds, coef, rmax, K, options, label, fill=(0, 0, 0.0), want_kernel=3):
    """One call under `options` (kernel = 3 added) against the oracle: tie-aware parity and the exact counters."""
    got, st = _run_gpu(indptr, indices, seeds, coef, rmax, K, fill=fill, options=dict(options, kernel=3))
    if want_kernel == 3:
        _ran_dense(st, label)
    else:
        assert st["kernel"] == want_kernel and st["failed_rows"] == 0, (label, st["kernel"])
    exp, ost = _oracle(indptr, indices, seeds, coef, rmax, K, fill=fill)
    rep = _assert_parity(seeds, K, got, exp, fill=fill if fill != (0, 0, 0.0) else None, next_value=ost["next_value"], label=label)
    if want_kernel == 3:
        _exact_counters(st, ost, label)
    return got, st, rep


# ---------------------------------------------------------------- 1. known-answer rows
@pytest.mark.parametrize("seeds,K,rmax,coef", [
    ([0, 3, 2, 0], 4, 0.0, KAT_COEF), ([0], 2, 0.0, KAT_COEF), ([0], 4, 0.3, KAT_COEF), ([0], 4, 0.6, KAT_COEF),
    ([0], 4, 0.0, np.array([1.0])), ([0, 1], 1, 0.0, KAT_COEF),
])
@pytest.mark.parametrize("csr", [0, 1])
def test_kat(seeds, K, rmax, coef, csr):
    got, st, _ = _against_oracle(KAT_INDPTR, KAT_INDICES, seeds, coef, rmax, K, {"dn_csr_lds": csr}, "", fill=FILL)
    if list(seeds) == [0, 3, 2, 0]:                                    # the hand-derived values of SURVEY.md A.3
        assert got[1][:3].tolist() == [0, 2, 1]                        # by value, descending
        assert dict(zip(got[1][:3].tolist(), got[2][:3].tolist())) == pytest.approx({0: 9 / 14, 2: 3 / 14, 1: 1 / 7}, rel=1e-15)
        assert got[1][3] == -1 and got[2][3] == -1.0 and got[0][3] == -1          # 4th slot untouched
        assert got[1][4] == 3 and got[2][4] == 1.0
        assert got[1][8] == 2 and got[2][8] == 1.0                     # dangling seed keeps its mass
        assert got[1][12:15].tolist() == [0, 2, 1]                     # the duplicate seed, on whatever state its workgroup had


def test_one_node_without_edges():
    indptr, indices = np.array([0, 0], np.int32), np.array([], np.int32)
    for K in (1, 3):
        got, st, _ = _against_oracle(indptr, indices, [0, 0], KAT_COEF, 0.0, K, {}, "one node", fill=FILL)
        for i in range(2):
            assert (got[0][i * K], got[1][i * K], got[2][i * K]) == (0, 0, 1.0)
            assert (got[1][i * K + 1:(i + 1) * K] == -1).all()


# ---------------------------------------------------------------- 2. golden rows of the real reference
def _golden(name, mode):
    if (name, mode) not in _cache:
        z = np.load(os.path.join(GOLD, f"{name}.npz"))
        rmax, K = float(z[f"{mode}_params"][0]), int(z[f"{mode}_params"][1])
        seeds = z["seeds"][:256].astype(np.int32)
        exp = tuple(z[f"{mode}_{a}"][:256 * K] for a in ("row", "col", "val"))
        _, ost = _oracle(z["indptr"], z["indices"], seeds, z[f"{mode}_coef"], rmax, K)
        _cache[(name, mode)] = (z["indptr"], z["indices"], seeds, z[f"{mode}_coef"], rmax, K, exp, ost)
    return _cache[(name, mode)]


@pytest.mark.parametrize("name", ["cora", "citeseer"])
@pytest.mark.parametrize("mode", ["ppr", "avg", "single"])
def test_reference_golden_rows(name, mode):
    indptr, indices, seeds, coef, rmax, K, exp, ost = _golden(name, mode)
    for csr in (0, 1):
        for block in (256, 1024):
            label = f"dense {name}/{mode} csr_lds {csr} x{block}"
            got, st = _run_gpu(indptr, indices, seeds, coef, rmax, K, options={"kernel": 3, "dn_csr_lds": csr, "dn_block_threads": block})
            _ran_dense(st, label)
            assert st["block_threads"] == block and st["lds_levels"] > 0
            rep = _assert_parity(seeds, K, got, exp, next_value=ost["next_value"], max_tie_frac=0.60 if mode == "single" else 0.30, label=label)
            print(f"[dense] {label}: lds_bytes {st['lds_bytes']} workgroups {st['workgroups']} max rel err {rep.max_rel_err:.3e} "
                  f"tie rows {rep.tie_rows} max_level_edges {st['max_level_edges']} {st['kernel_ms']:.2f} ms")
            assert rep.max_rel_err < 1e-12
            _exact_counters(st, ost, label)
            assert 0 < st["max_level_edges"] <= len(indices)


# ---------------------------------------------------------------- 3. the push test at its threshold
@pytest.mark.parametrize("name", [n for n in pb.GPU_CASES if n != "l2_wide"])
def test_push_threshold(name):
    case = PB_CASES[name]
    assert case.n_nodes <= CAP
    widths = case.degree_bits + ((31, 0) if case.path == "saturation" else ())
    for bits in widths:
        extra = {} if bits == 31 else {"max_degree_bits": bits}
        for K, pos in sorted(case.full_groups().items()):
            for csr in (0, 1):
                st = _run_push(case, pos, K, dict(extra, kernel=3, dn_csr_lds=csr), 3, f"{name} dense K{K} bits{bits} csr_lds {csr}")
                walks = [pb.push_walk64(case.indptr, case.indices, case.seeds[p], case.coef, case.rmax) for p in pos]
                assert st["support"] == sum(len(w.reserve) for w in walks) and st["frontier"] == sum(w.frontier_sum for w in walks)


def test_a_graph_above_the_cap_runs_what_kernel_0_would():
    case = PB_CASES["l2_wide"]
    assert case.n_nodes > CAP
    for K, pos in sorted(case.full_groups().items()):
        _run_push(case, pos, K, {"kernel": 3}, 1, f"l2_wide kernel 3 K{K}")


# ---------------------------------------------------------------- 4. the select at the K-th place
@pytest.mark.parametrize("name", sb.GPU_CASES)
def test_select_is_strict(name):
    case = SB_CASES[name]
    indptr, indices, seeds, ids = case.compact(limit=CAP)
    for K in case.ks:
        for opts in ({}, {"dn_csr_lds": 1}, {"dn_block_threads": 256}, {"dn_block_threads": 1024}):
            label = f"{name} dense K{K} {opts}"
            got, st = _run_gpu(indptr, indices, seeds, case.coef, case.rmax, K, fill=FILL, options=dict(opts, kernel=3))
            _hold(case, K, got, st, 3, label, ids)


# ---------------------------------------------------------------- 5. edges of the kernel's own loops
def _ring(n):
    return np.arange(n + 1, dtype=np.int32), ((np.arange(n) + 1) % n).astype(np.int32)


def _digraph(rng, n, mean_deg):
    deg = rng.poisson(mean_deg, n)
    deg[rng.integers(0, n, max(1, n // 16))] = 0                       # dangling nodes
    deg[int(rng.integers(0, n))] = n // 2                              # one hub
    indptr = np.zeros(n + 1, np.int32)
    np.cumsum(deg, out=indptr[1:])
    return indptr, rng.integers(0, n, int(indptr[-1])).astype(np.int32)          # repeated, unsorted columns


def test_ring_at_the_cap_and_one_above():
    from grand_plus_amd.recipes import make_coef
    coef = make_coef("ppr", 4, 0.2)
    indptr, indices = _ring(CAP)
    for csr in (0, 1):
        got, st, _ = _against_oracle(indptr, indices, [0, CAP - 1], coef, 0.0, 8, {"dn_csr_lds": csr}, f"ring {CAP} csr_lds {csr}", fill=FILL)
        assert got[1][:6].tolist() == [0, 1, 2, 3, 4, -1] and got[1][8:14].tolist() == [CAP - 1, 0, 1, 2, 3, -1]
    indptr, indices = _ring(CAP + 1)
    _against_oracle(indptr, indices, [0, CAP], coef, 0.0, 8, {}, f"ring {CAP + 1}", fill=FILL, want_kernel=1)


@pytest.mark.parametrize("n,block", [(63, 0), (64, 0), (65, 0), (255, 256), (257, 256), (511, 512), (513, 512), (1023, 1024), (1025, 1024)])
def test_node_counts_around_chunk_and_block(n, block):
    from grand_plus_amd.recipes import make_coef
    rng = np.random.default_rng(n)
    indptr, indices = _digraph(rng, n, 3.0)
    seeds = np.concatenate([[0, n - 1, n - 1], rng.integers(0, n, 29)]).astype(np.int32)
    for csr in (0, 1):
        opts = {"dn_csr_lds": csr, "max_workgroups": 3}
        if block:
            opts["dn_block_threads"] = block
        _, st, _ = _against_oracle(indptr, indices, seeds, make_coef("ppr", 5, 0.3), 1e-4, 16, opts, f"n {n} x{block} csr_lds {csr}")
        assert st["block_threads"] == (block or 512)


def test_star_hub_of_cap_leaves_is_one_wave_edge_range():
    """The hub's cap - 1 edges are one pusher of one chunk: its wave walks them 64 at a time."""
    n = CAP
    indptr = np.concatenate([[0], np.arange(n - 1, 2 * n - 1)]).astype(np.int32)          # 0 -> every leaf, every leaf -> 0
    indices = np.concatenate([np.arange(1, n), np.zeros(n - 1)]).astype(np.int32)
    for csr in (0, 1):
        got, st, _ = _against_oracle(indptr, indices, [0, 5, n - 1], pb.dyadic_coef(4), 0.0, 16, {"dn_csr_lds": csr}, f"star csr_lds {csr}")
        assert st["max_level_edges"] == n - 1 and st["edges"] > 3 * (n - 1)
        assert got[1][0] == 0 and got[1][1:16].tolist() == list(range(1, 16))            # the leaves tie: columns ascending


def test_unsorted_and_repeated_columns():
    indptr = np.array([0, 3, 5, 6], np.int32); indices = np.array([2, 1, 1, 0, 0, 2], np.int32)
    for csr in (0, 1):
        _against_oracle(indptr, indices, [0, 1, 2], KAT_COEF, 0.0, 3, {"dn_csr_lds": csr}, "unsorted rows")


def _tiny():
    from grand_plus_amd import synth
    if "tiny" not in _cache:
        indptr, indices = synth.shape_csr("tiny")
        _cache["tiny"] = (indptr, indices, synth.seeds(len(indptr) - 1, 96))
    return _cache["tiny"]


@pytest.mark.parametrize("K", [1, 7, 64, 1000])
def test_k_extremes(K):
    from grand_plus_amd.recipes import make_coef
    indptr, indices, seeds = _tiny()
    _against_oracle(indptr, indices, seeds, make_coef("ppr", 5, 0.3), 1e-4, K, {}, f"tiny K{K}")


def test_k_above_the_node_count():
    rng = np.random.default_rng(7)
    indptr, indices = _digraph(rng, 40, 3.0)
    got, st, _ = _against_oracle(indptr, indices, np.arange(40, dtype=np.int32), pb.dyadic_coef(5), 0.0, 64, {}, "K > N", fill=FILL)
    assert (got[1].reshape(40, 64)[:, 40:] == -1).all()


def test_rmax_zero_whole_graph_support():
    from grand_plus_amd.recipes import make_coef
    indptr, indices, seeds = _tiny()
    got, st, _ = _against_oracle(indptr, indices, seeds[:64], make_coef("avg", 6), 0.0, 1024, {}, "tiny rmax 0")
    assert st["support"] > 64 * 1024                                   # supports reach well past K


# ---------------------------------------------------------------- 6. rows after rows
def test_rows_after_rows_on_two_workgroups():
    import torch
    from grand_plus_amd import Graph
    from grand_plus_amd.parity import TAU_VAL
    from grand_plus_amd.recipes import make_coef
    indptr, indices, seeds = _tiny()
    seeds = seeds.astype(np.int32).copy()
    seeds[1::7] = seeds[0]                                             # duplicates
    coef, rmax, K = make_coef("ppr", 5, 0.3), 1e-4, 32
    S = len(seeds)
    opts = {"max_workgroups": 2}
    got, st, _ = _against_oracle(indptr, indices, seeds, coef, rmax, K, opts, "rows after rows", fill=FILL)
    assert st["workgroups"] == 2                                       # 48 rows each
    rows = {}
    for i, s in enumerate(seeds.tolist()):
        row = dict(zip(got[1][i * K:(i + 1) * K].tolist(), got[2][i * K:(i + 1) * K].tolist()))
        if s in rows:                                                  # a duplicate seed, behind other rows of its workgroup
            assert row.keys() == rows[s].keys() and all(abs(row[c] - rows[s][c]) <= TAU_VAL * rows[s][c] for c in row if c >= 0)
        rows[s] = row
    # the same rows in another order
    perm = np.random.default_rng(3).permutation(S)
    again, st2 = _run_gpu(indptr, indices, seeds[perm], coef, rmax, K, fill=FILL, options=dict(opts, kernel=3))
    _ran_dense(st2)
    for j, i in enumerate(perm.tolist()):
        row = dict(zip(again[1][j * K:(j + 1) * K].tolist(), again[2][j * K:(j + 1) * K].tolist()))
        exp = rows[int(seeds[i])]
        assert row.keys() == exp.keys() and all(abs(row[c] - exp[c]) <= TAU_VAL * exp[c] for c in row if c >= 0), (i, j)
    # the device API on a side stream, with a `filled` array
    g = Graph(indptr, indices, 0)
    for k, v in dict(opts, kernel=3).items():
        g.set_option(k, v)
    side = torch.cuda.Stream()
    d_row = torch.full((S * K,), FILL[0], dtype=torch.int32, device="cuda")
    d_col = torch.full((S * K,), FILL[1], dtype=torch.int32, device="cuda")
    d_val = torch.full((S * K,), FILL[2], dtype=torch.float64, device="cuda")
    d_fill = torch.full((S,), -7, dtype=torch.int32, device="cuda")
    d_seeds = torch.from_numpy(seeds).cuda()
    torch.cuda.synchronize()
    g.gfpush_device(d_seeds, coef, rmax, K, d_row, d_col, d_val, d_fill, stream=side.cuda_stream)
    st3 = g.stats()
    g.close()
    _ran_dense(st3)
    filled = d_fill.cpu().numpy()
    assert filled.tolist() == [(got[1][i * K:(i + 1) * K] >= 0).sum() for i in range(S)] and st3["filled"] == filled.sum()
    dev = (d_row.cpu().numpy(), d_col.cpu().numpy(), d_val.cpu().numpy())
    exp, ost = _oracle(indptr, indices, seeds, coef, rmax, K, fill=FILL)
    _assert_parity(seeds, K, dev, exp, fill=FILL, next_value=ost["next_value"])
    # the host merge of the pinned slab, every merged row verified
    _against_oracle(indptr, indices, seeds, coef, rmax, K, dict(opts, verify_merge=1), "verify_merge", fill=FILL)


# ---------------------------------------------------------------- 7. the default is untouched
def test_nothing_set_never_runs_the_dense_kernel():
    from grand_plus_amd import Graph
    from grand_plus_amd.recipes import make_coef
    z = np.load(os.path.join(GOLD, "cora.npz"))
    indptr, indices, seeds = _tiny()
    for ip, ix, sd in ((z["indptr"], z["indices"], z["seeds"][:64].astype(np.int32)), (indptr, indices, seeds)):
        _, st = _run_gpu(ip, ix, sd, make_coef("ppr", 5, 0.3), 1e-4, 16)
        assert st["kernel"] in (1, 2)
    g = Graph(indptr, indices, 0)
    with pytest.raises(ValueError):
        g.set_option("kernel", 4)
    with pytest.raises(ValueError):
        g.set_option("dn_block_threads", 768)
    g.close()
