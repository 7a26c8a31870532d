"""GPU tests that hold GFPush's top-K select (graph.h:111-126) at the K-th place in both kernels, on the graphs of
tests/select_boundary_cases.py (audited on the CPU by tests/test_host_select_boundary.py: every case is exact, holds the tie,
ulp distance or counter edge it claims, and is moved by a deliberate mistake of the select rule).

Every run is held to the header's promise with NO tolerance: slots 0 .. filled-1 of a row hold the positive totals by (value
desc, column asc) -- the same column in the same slot, the value bit-equal -- and every slot from `filled` on keeps the
caller's fill.  No tie row is forgiven and no row is left out.  The forgiving comparator runs as well and must report exactly
the tie rows in which the ORACLE's choice among equal totals differs from the header's.

Which copy of the rule a run reaches, and by what that is known:
  sketch kernel (kernel = 2)    st["kernel"]; both workgroup shapes; the reserve sketch at its default size and at 2^8 cells
                                (sk_lg_mr = 8: collisions lift cells, more nodes reach a round); the first cut at its default
                                rank and at rank 3 (sk_target = 3: a cut so high that fewer than K nodes pass it --
                                st["sketch_second_sweeps"] > 0); TOP-K's partitions by the overflow counter diag_sub[10].
  general kernel (kernel = 1)   st["kernel"]; the self-addressed CSR (ranks by unit number) or the packed one (gk_acsr); the
                                pruned or the full aggregation (exact_stats: st["support"] tells them apart where a node goes
                                unclaimed); LDS or HBM level tables (force_global: st["global_levels"]); direct-indexed tables
                                on the graph without its padding (direct_tables); 512, 768 and 1024 threads; a 44 KB table
                                (the aggregation runs in hash partitions, big_cap shrinks below the tie group).
No counter tells a compacted bucket from one that stays in HBM, a binade first digit from a 4096-bin one, or the sketch
select's value bytes from its id bytes: for these every setting runs and every one must equal the reference."""
import numpy as np
import pytest

import select_boundary_cases as sb
from test_gpu_parity import _assert_parity, _oracle, _run_gpu

pytestmark = pytest.mark.gpu

CASES = sb.cases()
FILL = (-1, -1, -1.0)

# (sk_block_threads, sk_lg_mr, sk_target); 0 = the default
SK_RUNS = [(768, 0, 0), (768, 8, 0), (768, 0, 3), (768, 8, 3), (512, 0, 0), (512, 8, 0), (512, 0, 3), (512, 8, 3)]
# (gk_acsr, exact_stats, force_global)
GK_RUNS = [(1, 0, 0), (1, 1, 0), (0, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1)]
GK_BLOCKS = (512, 768, 1024)
SMALL_LDS = {"block_threads": 256, "lds_bytes": 45056}

_cache = {}


def _reference(case, K, ids=None):
    """(rows, col, val, filled per row) the header promises under fill FILL; ids: the node ids of a compacted graph."""
    key = (case.name, K, ids is not None)
    if key not in _cache:
        S = len(case.seeds)
        col = np.full(S * K, FILL[1], np.int32)
        val = np.full(S * K, FILL[2], np.float64)
        row = np.full(S * K, FILL[0], np.int32)
        filled = []
        back = None if ids is None else {int(v): i for i, v in enumerate(ids)}
        for i, exp in enumerate(case.expected(K)):
            for j, (c, v) in enumerate(exp):
                col[i * K + j] = c if back is None else back[c]
                val[i * K + j] = v
                row[i * K + j] = case.seeds[i] if back is None else back[int(case.seeds[i])]
            filled.append(len(exp))
        _cache[key] = (row, col, val, filled)
    return _cache[key]


def _oracle_rows(case, K):
    key = ("oracle", case.name, K)
    if key not in _cache:
        exp, ost = _oracle(case.indptr, case.indices, case.seeds, case.coef, case.rmax, K, fill=FILL)
        _, col, _, filled = _reference(case, K)
        ties = sum(set(exp[1][i * K:i * K + f].tolist()) != set(col[i * K:i * K + f].tolist()) for i, f in enumerate(filled))
        _cache[key] = (exp, ost, ties)
    return _cache[key]


def _hold(case, K, got, st, want_kernel, label, ids=None):
    """The strict comparison of one call's three arrays."""
    row, col, val, filled = _reference(case, K, ids)
    assert st["kernel"] == want_kernel, (label, st["kernel"])
    assert st["failed_rows"] == 0 and st["retried_rows"] == 0, (label, st["failed_rows"], st["retried_rows"], st["diag_sub"][:8])
    assert st["filled"] == sum(filled), (label, st["filled"], filled)
    for i, f in enumerate(filled):
        g_col, g_val = got[1][i * K:(i + 1) * K], got[2][i * K:(i + 1) * K]
        e_col, e_val = col[i * K:(i + 1) * K], val[i * K:(i + 1) * K]
        if not (np.array_equal(g_col, e_col) and np.array_equal(g_val.view(np.int64), e_val.view(np.int64))):
            same_set = set(zip(g_col[:f].tolist(), g_val[:f].view(np.int64).tolist())) == set(zip(e_col[:f].tolist(), e_val[:f].view(np.int64).tolist()))
            same_cols = set(g_col[:f].tolist()) == set(e_col[:f].tolist())
            kind = "a wrong ORDER" if same_set else "a changed BIT" if same_cols else "a wrong SET"
            j = int(np.flatnonzero((g_col != e_col) | (g_val.view(np.int64) != e_val.view(np.int64)))[0])
            raise AssertionError(f"{label}: row {i} (K {K}, filled {f}): {kind}; first at slot {j}: got ({g_col[j]}, {g_val[j]!r}), "
                                 f"expected ({e_col[j]}, {e_val[j]!r})")
        assert np.array_equal(got[0][i * K:(i + 1) * K], row[i * K:(i + 1) * K]), (label, i)


def _strict(case, K, options, want_kernel, label="", compacted=False, twice=False):
    """One call through gfpush_omp under fill (-1, -1, -1.0), held strictly; on the padded graph the forgiving comparator runs
    too.  twice: the call is repeated and must give the same bytes.  Returns the stats."""
    label = label or f"{case.name} K{K} {options}"
    if compacted:
        indptr, indices, seeds, ids = case.compact()
    else:
        indptr, indices, seeds, ids = case.indptr, case.indices, case.seeds, None
    got, st = _run_gpu(indptr, indices, seeds, case.coef, case.rmax, K, fill=FILL, options=options)
    print(f"[select boundary] {label}: kernel {st['kernel']} x{st['block_threads']} filled {st['filled']} support {st['support']} "
          f"second sweeps {st['sketch_second_sweeps']} topk overflows {st['diag_sub'][10]} lds_levels {st['lds_levels']} "
          f"global_levels {st['global_levels']} {st['kernel_ms']:.2f} ms")
    _hold(case, K, got, st, want_kernel, label, ids)
    if not compacted:
        exp, ost, ties = _oracle_rows(case, K)
        rep = _assert_parity(seeds, K, got, exp, fill=FILL, next_value=ost["next_value"])
        assert rep.tie_rows == ties, (label, rep.tie_rows, ties)
    if twice:
        again, _ = _run_gpu(indptr, indices, seeds, case.coef, case.rmax, K, fill=FILL, options=options)
        for a, b in zip(got, again):
            assert a.tobytes() == b.tobytes(), label
    return st


@pytest.mark.parametrize("name", [n for n in sb.GPU_CASES if 2 in CASES[n].kernels])
def test_sketch_kernel_select(name):
    case = CASES[name]
    for K in case.ks:
        sweeps = {}
        for block, lg_mr, target in SK_RUNS:
            opts = {"kernel": 2, "sk_block_threads": block}
            if lg_mr:
                opts["sk_lg_mr"] = lg_mr
            if target:
                opts["sk_target"] = target
            st = _strict(case, K, opts, 2, twice=(lg_mr, target) == (0, 0))
            assert st["block_threads"] == block
            sweeps[(block, lg_mr, target)] = st["sketch_second_sweeps"]
        rows = len(case.seeds)
        for block in (768, 512):
            if case.path == "tie" and name != "tie_g5000":            # the first cut already proves the row complete
                assert sweeps[(block, 0, 0)] == 0, (name, K, sweeps)
            if case.path == "near":                                   # 296 nodes within 2^12 ulps of the K-th: one more sweep
                assert sweeps[(block, 0, 0)] > 0, (name, K, sweeps)
            if case.path in ("tie", "near"):                          # a cut at rank 3 leaves fewer than K nodes: t_c >> 4 ...
                assert sweeps[(block, 0, 3)] > 0, (name, K, sweeps)
                if K >= 64 and name != "tie_g5000":                   # ... twice, and then t_c = 1
                    assert sweeps[(block, 0, 3)] == 3 * rows, (name, K, sweeps)


@pytest.mark.parametrize("name", sb.GPU_CASES)
def test_general_kernel_select(name):
    case = CASES[name]
    small = case.compact() is not None
    for K in case.ks:
        support = {}
        for acsr, exact, glob in GK_RUNS:
            opts = {"kernel": 1, "gk_acsr": acsr, "exact_stats": exact, "force_global": glob}
            st = _strict(case, K, opts, 1, twice=(acsr, exact, glob) == (1, 0, 0))
            assert (st["global_levels"] > 0) == bool(glob), (name, opts, st["global_levels"])
            support[(acsr, exact, glob)] = st["support"]
        for acsr, glob in ((1, 0), (0, 0), (0, 1)):
            assert support[(acsr, 0, glob)] <= support[(acsr, 1, glob)], (name, K, support)
        if case.path == "prune":                                      # Z and its like own no record at tau / n_levels: never claimed
            assert support[(1, 0, 0)] < support[(1, 1, 0)] and support[(0, 0, 0)] < support[(0, 1, 0)], support
        for block in GK_BLOCKS:
            for exact in (0, 1):
                _strict(case, K, {"kernel": 1, "block_threads": block, "exact_stats": exact}, 1)
                if small and block != 1024:
                    for direct in (1, 0):
                        _strict(case, K, {"kernel": 1, "block_threads": block, "exact_stats": exact, "direct_tables": direct}, 1, compacted=True)
        if case.path in ("tie", "near", "prune", "heavy"):
            for exact in (0, 1):
                for acsr in (1, 0):
                    _strict(case, K, dict(SMALL_LDS, kernel=1, exact_stats=exact, gk_acsr=acsr), 1)


def test_sketch_kernel_topk_partitions_keep_the_order():
    """The 5 000-member group and its hub's other leaves outgrow TOP-K's aggregation table when the cut lets every node through
    (sk_target = 4096): the table is refilled in 2, 4, ... hash partitions, the members fall into all of them, each partition's K
    best are merged with the running list."""
    case = CASES["tie_g5000"]
    for block in (768, 512):
        for lg_mr in (0, 8):
            opts = {"kernel": 2, "sk_block_threads": block, "sk_target": 4096}
            if lg_mr:
                opts["sk_lg_mr"] = lg_mr
            st = _strict(case, case.ks[0], opts, 2, twice=True)
            assert st["diag_sub"][10] > 0, (opts, st["diag_sub"][:12])


DOOR_CASES = ("tie_g257", "tie_step256_high", "near_bit0", "near_bit4")


@pytest.mark.parametrize("name", DOOR_CASES)
@pytest.mark.parametrize("kernel", [1, 2])
def test_same_contract_through_the_other_doors(name, kernel):
    """The device API (rows stay on the GPU, d_filled), the host path with verify_merge = 1, and the sharded handle with two parts
    on one device: the same slots, bit for bit.  Rows are doubled (a duplicate seed is legal) so that every part gets some."""
    import torch
    from grand_plus_amd import Graph
    case = CASES[name]
    K = case.ks[0]
    row, col, val, filled = _reference(case, K)
    S = len(case.seeds)
    # device API
    g = Graph(case.indptr, case.indices, 0)
    g.set_option("kernel", kernel)
    d_row = torch.full((S * K,), FILL[0], dtype=torch.int32, device="cuda")
    d_col = torch.full((S * K,), FILL[1], dtype=torch.int32, device="cuda")
    d_val = torch.full((S * K,), FILL[2], dtype=torch.float64, device="cuda")
    d_fill = torch.full((S,), -7, dtype=torch.int32, device="cuda")
    g.gfpush_device(torch.from_numpy(case.seeds).cuda(), case.coef, case.rmax, K, d_row, d_col, d_val, d_fill)
    st = g.stats()
    g.close()
    assert d_fill.cpu().tolist() == filled
    _hold(case, K, (d_row.cpu().numpy(), d_col.cpu().numpy(), d_val.cpu().numpy()), st, kernel, f"{name} device API kernel {kernel}")
    # host path, every merged row verified
    _strict(case, K, {"kernel": kernel, "verify_merge": 1}, kernel, f"{name} verify_merge kernel {kernel}")
    # two parts on one device
    seeds2 = np.concatenate([case.seeds, case.seeds])
    g = Graph(case.indptr, case.indices, 0, devices=[0, 0])
    for k, v in (("min_rows_per_gpu", 1), ("measure_choice", 0), ("kernel", kernel)):
        g.set_option(k, v)
    out = (np.full(2 * S * K, FILL[0], np.int32), np.full(2 * S * K, FILL[1], np.int32), np.full(2 * S * K, FILL[2]))
    g.gfpush_omp(seeds2, out[0], out[1], out[2], case.coef, case.rmax, K)
    st = g.stats()
    g.close()
    assert st["rows"] == 2 * S and st["failed_rows"] == 0 and st["filled"] == 2 * sum(filled)
    for a, e in zip(out, (row, col, val)):
        assert a.tobytes() == np.concatenate([e, e]).tobytes(), (name, kernel)
