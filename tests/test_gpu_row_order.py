"""GPU tests of option "row_order" (the pre-pass that hands the rows of a call out heaviest first: row_cost_kernel,
row_order_kernel, the row queue's row_map): whatever the order, every row is the oracle's and arrives exactly once.

Both kernels are forced (kernel = 2 / 1), both orders run, on the `small` synthetic shape with the MAG recipe and on the Pubmed
fixture with its own.  One oracle run per graph over a base list of seeds (random nodes, the largest hubs, degree-1 nodes);
every case indexes that list, so the expected rows are gathered, not recomputed.  Position -1 / -2 in a case stands for the
invalid seeds -1 / n_nodes, which only the device API lets through."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
SENTINEL = -7
N_RANDOM, N_HUBS, N_LEAVES = 960, 20, 20


@functools.lru_cache(maxsize=None)
def _base(name):
    """(indptr, indices, coef, rmax, K, base seeds, expected rows (row, col, val) as [len(base), K], next_value, filled)."""
    from grand_plus_amd import synth
    from grand_plus_amd.recipes import RECIPES
    from oracle import pyoracle
    if name == "small":
        indptr, indices = synth.shape_csr("small")
        r = RECIPES[("mag", "ppr")]
    else:
        z = np.load(os.path.join(GOLD, "pubmed.npz"))
        indptr, indices = z["indptr"], z["indices"]
        r = RECIPES[("pubmed", "ppr")]
    n = len(indptr) - 1
    deg = np.diff(indptr)
    by_deg = np.argsort(deg, kind="stable")
    leaves = by_deg[deg[by_deg] >= 1][:N_LEAVES]                       # the smallest non-dangling degrees (1 or 2: the self-loop counts)
    base = np.concatenate([synth.seeds(n, N_RANDOM), by_deg[-N_HUBS:], leaves]).astype(np.int32)
    K = r.top_k
    row, col, val, st = pyoracle.gfpush(indptr, indices, base, r.coef(), r.rmax, K, want_next=True)
    exp = tuple(a.reshape(len(base), K) for a in (row, col, val))
    return indptr, indices, r.coef(), r.rmax, K, base, exp, np.asarray(st["next_value"]), (exp[2] > 0).sum(axis=1)


HUB0, LEAF0 = N_RANDOM, N_RANDOM + N_HUBS                              # positions of the hubs / the leaves in the base list


def _run(name, pos, kernel, row_order, options=None, workgroups=None, stats=True):
    """One gfpush_device call over base[pos] with `filled` pre-filled with a sentinel; checks every row against the oracle's,
    `filled` of every row, and the device's order against the restated cost classes.  Returns the statistics."""
    import torch
    from grand_plus_amd import Graph
    from grand_plus_amd.parity import compare_rows
    from grand_plus_amd.row_cost import cost_class, row_costs
    indptr, indices, coef, rmax, K, base, exp, next_value, exp_filled = _base(name)
    n = len(indptr) - 1
    pos = np.asarray(pos, np.int64)
    S = len(pos)
    valid = pos >= 0
    seeds = np.where(valid, base[np.maximum(pos, 0)], np.where(pos == -1, -1, n)).astype(np.int32)
    g = Graph(indptr, indices, 0)
    opts = dict(kernel=kernel, row_order=row_order, measure_choice=0)
    if workgroups:
        opts["max_workgroups"] = workgroups
    opts.update(options or {})
    for k, v in opts.items():
        g.set_option(k, v)
    filled = torch.full((S,), SENTINEL, dtype=torch.int32, device="cuda")
    row, col, val, filled = g.gfpush_device(torch.from_numpy(seeds).cuda(), coef, rmax, K, filled=filled)
    torch.cuda.synchronize()
    order, shift, sat = g.row_order()
    st = g.stats() if stats and valid.all() else None                    # (stats() raises on an out-of-range seed: a failed row)
    g.close()
    f = filled.cpu().numpy()
    got = tuple(t.cpu().numpy().reshape(S, K) for t in (row, col, val))
    label = f"{name} kernel {kernel} row_order {row_order} S {S} {options or ''}"
    # every row was written exactly as the oracle has it (the sentinel gone = `order` reached every row)
    assert not (f == SENTINEL).any(), (label, np.flatnonzero(f == SENTINEL)[:8])
    assert (f[~valid] == 0).all(), label
    assert (f[valid] == exp_filled[pos[valid]]).all(), label
    for a in got:
        assert not a[~valid].any(), label                                # an invalid seed's slots keep their contents
    keep = np.arange(K)[None, :] < f[:, None]
    got = tuple(np.where(keep, a, 0)[valid].reshape(-1) for a in got)
    want = tuple(a[pos[valid]].reshape(-1) for a in exp)
    rep = compare_rows(seeds[valid], K, got, want, next_value=next_value[pos[valid]])
    assert rep.ok, label + "\n" + "\n".join(rep.messages)
    assert rep.exact_index_rows + rep.tie_rows == rep.rows == int(valid.sum())
    # the order: skipped in caller order and when every workgroup takes at most one row; else a permutation by class, descending
    if st is not None:
        assert st["kernel"] == kernel, (label, st["kernel"])
        workgroups = st["workgroups"]
    if row_order == 0 or (workgroups is not None and S <= workgroups):
        assert len(order) == 0, (label, len(order))
    elif workgroups is not None:
        assert np.array_equal(np.sort(order), np.arange(S)), label
        cls = cost_class(row_costs(indptr, indices, seeds, rmax, sat))
        assert (np.diff(cls[order]) <= 0).all(), (label, cls[order][:32])
    return st


def _both_orders(name, pos, kernel, **kw):
    """The case in both orders; the exact work counters do not depend on the order."""
    a = _run(name, pos, kernel, 1, **kw)
    b = _run(name, pos, kernel, 0, **kw)
    if a is not None:
        for key in ("rows", "pushes", "edges", "filled"):
            assert a[key] == b[key], (key, a[key], b[key])
    return a, b


GRAPHS_KERNELS = [(g, k) for g in ("small", "pubmed") for k in (2, 1)]


@pytest.mark.parametrize("name,kernel", GRAPHS_KERNELS)
def test_around_one_row_per_workgroup(name, kernel):
    """S = 1 and S = workgroups - 1, workgroups, workgroups + 1 with eight workgroups: the edges of the skip rule."""
    for S in (1, 7, 8, 9):
        _both_orders(name, np.arange(S) * 37 % N_RANDOM, kernel, workgroups=8)


@pytest.mark.parametrize("name,kernel", GRAPHS_KERNELS)
def test_many_rows_per_workgroup(name, kernel):
    """1 000 rows on three workgroups: hundreds of rows each, hubs and degree-1 seeds among them (the column cap, saturated
    degree fields), every cost class in one call."""
    pos = np.arange(1000)
    a, _ = _both_orders(name, pos, kernel, workgroups=3)
    assert a["workgroups"] == 3 and a["rows"] == 1000


@pytest.mark.parametrize("name,kernel", GRAPHS_KERNELS)
def test_duplicate_seeds_and_one_cost_class(name, kernel):
    dup = np.concatenate([np.arange(40), np.arange(40), np.full(20, 5), [HUB0 + N_HUBS - 1] * 3])
    _both_orders(name, dup, kernel, workgroups=8)
    _both_orders(name, np.full(100, 11), kernel, workgroups=8)           # all one node: one class must still give a permutation


@pytest.mark.parametrize("name,kernel", GRAPHS_KERNELS)
def test_invalid_seeds_first_last_and_adjacent(name, kernel):
    """Seeds -1 and n_nodes through the device API: filled = 0, nothing dereferenced, every other row right."""
    body = np.arange(60) * 13 % N_RANDOM
    pos = np.concatenate([[-1, -2], body[:20], [-2, -1, -1], body[20:40], [-1], body[40:], [HUB0 + N_HUBS - 1, -2, -1]])
    _both_orders(name, pos, kernel, workgroups=8)
    _both_orders(name, np.array([-1, -2, -1, -2, -1, -2, -1, -2, -1, 3]), kernel, workgroups=8)


@pytest.mark.parametrize("name,kernel", GRAPHS_KERNELS)
def test_hub_seeds_and_degree_one_seeds_together(name, kernel):
    pos = np.concatenate([np.arange(HUB0, HUB0 + N_HUBS), np.arange(LEAF0, LEAF0 + N_LEAVES), np.arange(HUB0, HUB0 + N_HUBS)])
    np.random.default_rng(3).shuffle(pos)
    _both_orders(name, pos, kernel, workgroups=8)


@pytest.mark.parametrize("name,kernel", GRAPHS_KERNELS)
def test_rows_that_outgrow_their_slab_still_arrive_once(name, kernel):
    """est_level_edges = 64 (as test_gpu_sketch.py has it): the first launch hands (nearly) every row to the retry list, whose
    launches keep their own lists -- row numbers, not queue positions."""
    pos = np.arange(300)
    a, b = _both_orders(name, pos, kernel, workgroups=8, options={"est_level_edges": 64})
    if name == "small":
        assert a["retried_rows"] > len(pos) // 2 and b["retried_rows"] > len(pos) // 2, (a["retried_rows"], b["retried_rows"])


def test_first_call_large_enough_to_calibrate():
    """32 768 rows with nothing forced: the calibration's timing runs go through the pre-pass like any other call, and the call
    that follows returns the oracle's rows."""
    import torch
    from grand_plus_amd import Graph
    from grand_plus_amd.parity import compare_rows
    indptr, indices, coef, rmax, K, base, exp, next_value, exp_filled = _base("small")
    S = 32768
    pos = np.arange(S) % len(base)
    seeds = base[pos]
    g = Graph(indptr, indices, 0)
    g.set_option("row_order", 1)
    filled = torch.full((S,), SENTINEL, dtype=torch.int32, device="cuda")
    row, col, val, filled = g.gfpush_device(torch.from_numpy(seeds).cuda(), coef, rmax, K, filled=filled)
    st = g.stats()
    order, _, _ = g.row_order()
    g.close()
    assert st["choice_ms"][0] > 0 and st["choice_ms"][1] > 0, st["choice_ms"]
    assert np.array_equal(np.sort(order), np.arange(S))
    f = filled.cpu().numpy()
    assert (f == exp_filled[pos]).all()
    keep = (np.arange(K)[None, :] < f[:, None]).reshape(-1)
    got = tuple(np.where(keep, t.cpu().numpy(), 0) for t in (row, col, val))
    sub = slice(0, 4096 * K)                                             # (the Python comparator is the slow part: the first 4 096 rows row by row ...)
    rep = compare_rows(seeds[:4096], K, tuple(a[sub] for a in got), tuple(a[pos[:4096]].reshape(-1) for a in exp),
                       next_value=next_value[pos[:4096]])
    assert rep.ok, "\n".join(rep.messages)
    # (... and every repeat of a base seed against its first occurrence, as value multisets)
    v = np.sort(got[2].reshape(S, K), axis=1)
    assert np.allclose(v, v[pos], rtol=1e-12, atol=0.0)
