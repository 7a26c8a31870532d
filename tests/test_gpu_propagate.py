"""Parity of gp_propagate_features with the scipy float64 restatement of the
reference's predict() propagation.  Storage is fp32 (rounded once per step, fp64 sums): tolerance
|d| <= 2e-6*|ref| + 1e-6*max|ref| for up to 20 steps (propagate_cases.tolerance; tests/test_host_propagate.py shows
on the CPU that fp32 storage alone stays below 0.1 of it on every case of this file).

Covered: the citation graphs with their recipes; the Reddit shape's hubs; weighted edges and dangling rows; order 0;
fp32 drift after 20 steps; a multi-GPU handle; and, on the graphs of propagate_cases.py,
  * rows of exactly 4096 / 4097 / 4227 / 5999 / 4104 neighbours (both sides of kLongRow, the long kernel's tail loop)
    in every mode, weighted and not, each asserted by name, and a row whose weights sum to 0;
  * every vector width and lane-group size, one and several column trips, the datasets' own widths (500, 602, 1433);
  * the grid-stride loops of both SpMM kernels;
  * bitwise determinism, out=, a side stream, inputs left intact, alpha at 0 and 1;
  * propagate_features and both GFPush kernels on one handle, in either order;
  * argument errors, a bad `out` included."""
import os

import numpy as np
import pytest

import propagate_cases as pc

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _assert_close(got, ref, rows=None):
    """propagate_cases.tolerance per element (a NaN is off); `rows` = {row: label} are asserted first, by name."""
    tol = pc.tolerance(ref)
    bad = ~(np.abs(got - ref) <= tol)
    for u, label in (rows or {}).items():
        assert not bad[u].any(), (f"row {u} ({label}): {bad[u].sum()} of {bad[u].size} elements off; "
                                  f"max abs err {np.abs(got[u] - ref[u]).max():.3e}, tolerance from {tol[u].min():.3e}")
    assert not bad.any(), f"{bad.sum()} of {bad.size} elements off; max abs err {np.abs(got - ref).max():.3e}"


def _check(indptr, indices, F, mode, order, alpha, weights=None, seed=0, out=None, stream=None, g=None, X=None, ref=None,
           rows=None):
    """One propagate_features call against oracle.predict_ref.propagate_ref; returns the tensor the call returned.
    g / X / ref: a handle, features and a reference the caller already has; stream: a torch.cuda.Stream to run under."""
    import scipy.sparse as sp
    import torch
    from grand_plus_amd import Graph
    from oracle.predict_ref import propagate_ref
    n = len(indptr) - 1
    if X is None:
        X = np.random.default_rng(seed).standard_normal((n, F)).astype(np.float32)
    if ref is None:
        data = np.ones(len(indices)) if weights is None else weights.astype(np.float64)
        ref = propagate_ref(sp.csr_matrix((data, indices, indptr), shape=(n, n)), X, mode, order, alpha)
    if g is None:
        g = Graph(indptr, indices, 0)
    w = None if weights is None else torch.tensor(weights.astype(np.float32)).cuda()
    x = torch.tensor(X).cuda()
    if stream is None:
        got = g.propagate_features(x, mode, order, alpha, edge_weight=w, out=out)
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            got = g.propagate_features(x, mode, order, alpha, edge_weight=w, out=out)
        stream.synchronize()
    _assert_close(got.cpu().numpy(), ref, rows)
    return got


def _check_case(case, **kw):
    indptr, indices, w, X = pc.inputs(case)
    return _check(indptr, indices, case.F, case.mode, case.order, case.alpha, weights=w, X=X, ref=pc.reference(case), **kw)


@pytest.mark.parametrize("name,mode,order,alpha", [("cora", "ppr", 20, 0.2), ("cora", "avg", 4, 0.2), ("cora", "single", 2, 0.2),
                                                    ("pubmed", "ppr", 6, 0.5), ("citeseer", "avg", 2, 0.4)])
def test_citation_graphs(name, mode, order, alpha):
    z = np.load(os.path.join(GOLD, f"{name}.npz"))           # the adj + I CSR the reference's loader produces
    _check(z["indptr"], z["indices"], 96, mode, order, alpha)


@pytest.mark.parametrize("F", [1, 64, 100, 130])
def test_feature_widths_and_hubs(F):
    from grand_plus_amd import synth
    indptr, indices = synth.shape_csr("reddit")              # max degree 19k: exercises the long-row kernel
    _check(indptr, indices, F, "ppr", 3, 0.1, seed=F)


def test_weighted_edges_and_dangling_rows():
    rng = np.random.default_rng(3)
    n = 3000
    rows = [np.sort(rng.choice(n, size=(0 if u % 7 == 0 else int(rng.integers(1, 12))), replace=False)) for u in range(n)]
    indptr = np.zeros(n + 1, np.int32); indptr[1:] = np.cumsum([len(r) for r in rows])
    indices = np.concatenate(rows).astype(np.int32)
    w = rng.uniform(0.5, 2.0, size=len(indices))             # e.g. a diagonal stored as 2.0 when adj already had the loop
    for mode in ("ppr", "avg", "single"):
        _check(indptr, indices, 40, mode, 5, 0.3, weights=w)


def test_order_zero_and_errors():
    import torch
    from grand_plus_amd import synth
    from grand_plus_amd import Graph
    indptr, indices = synth.shape_csr("tiny")
    g = Graph(indptr, indices, 0)
    _check(indptr, indices, 32, "ppr", 0, 0.2, g=g)           # order 0: alpha * F
    _check(indptr, indices, 32, "avg", 0, 0.2)
    x = torch.zeros((len(indptr) - 1, 8), device="cuda")
    with pytest.raises(ValueError, match="Unknown propagation mode"):
        g.propagate_features(x, "heat", 2)
    with pytest.raises(ValueError):
        g.propagate_features(x[:5].contiguous(), "ppr", 2)
    with pytest.raises(TypeError):
        g.propagate_features(x.double(), "ppr", 2)


def test_fp32_storage_drift_after_20_steps_stays_below_1e_6():
    """the reference iterates in float64 (model.py:186-210) and casts once at the end (model.py:175);
    here the running state is rounded to fp32 after every step (sums are fp64).  The accumulated drift of that
    rounding after the longest shipped recipe (Cora ppr, order 20) and on the Pubmed graph at order 20:
    max |got - ref| <= 1e-6 * max |ref|, i.e. below the fp32 resolution of the result the reference itself returns."""
    import scipy.sparse as sp
    import torch
    from grand_plus_amd import Graph
    from oracle.predict_ref import propagate_ref
    for name, alpha in (("cora", 0.2), ("pubmed", 0.5)):
        z = np.load(os.path.join(GOLD, f"{name}.npz"))
        indptr, indices = z["indptr"], z["indices"]
        n = len(indptr) - 1
        X = np.random.default_rng(7).standard_normal((n, 64)).astype(np.float32)
        adj = sp.csr_matrix((np.ones(len(indices)), indices, indptr), shape=(n, n))
        ref = propagate_ref(adj, X, "ppr", 20, alpha)
        got = Graph(indptr, indices, 0).propagate_features(torch.from_numpy(X).cuda(), "ppr", 20, alpha).cpu().numpy()
        drift = np.abs(got - ref).max() / np.abs(ref).max()
        assert drift <= 1e-6, f"{name}: drift {drift:.2e}"
        assert np.abs(got - ref.astype(np.float32)).max() <= 4e-7 * np.abs(ref).max() + 1e-30


def test_multi_gpu_handle_propagates_on_its_first_gpu():
    """A multi-GPU handle owns no device memory itself (the CSR lives in its first part): propagate_features on it must
    give the single-GPU result instead of faulting on null pointers."""
    import scipy.sparse as sp
    import torch
    from grand_plus_amd import Graph
    from oracle.predict_ref import propagate_ref
    z = np.load(os.path.join(GOLD, "cora.npz"))
    indptr, indices = z["indptr"], z["indices"]
    n = len(indptr) - 1
    X = np.random.default_rng(3).standard_normal((n, 32)).astype(np.float32)
    ref = propagate_ref(sp.csr_matrix((np.ones(len(indices)), indices, indptr), shape=(n, n)), X, "ppr", 4, 0.2)
    g = Graph(indptr, indices, 0, n_gpus=0)
    got = g.propagate_features(torch.from_numpy(X).cuda(), "ppr", 4, 0.2).cpu().numpy()
    assert np.all(np.abs(got - ref) <= pc.tolerance(ref))
    g.close()


# ---------------------------------------------------------------- the graphs and cases of propagate_cases.py
BOUNDARY_ROWS = {u: f"degree {pc.HUB_DEGREES[u]}" for u in range(pc.N_BOUNDARY_ROWS)}


@pytest.mark.parametrize("case", pc.HUB_CASES, ids=str)
def test_hub_rows_in_every_mode_weighted_and_not(case):
    """Rows of 4096 (main kernel) and 4097 / 4227 / 5999 / 4104 neighbours (long kernel; 4227 = 4096 + 128 + 3 has a tail
    after the 128-neighbour batches), each asserted by name, then the whole matrix.  Weighted: one short row's weights
    sum to 0, its scale is 1 / 1e-12 and its result 0, not NaN; the weights of another sum to 1e-12 itself, where
    max(deg, 1e-12) and deg + 1e-12 differ by a factor of two."""
    rows = dict(BOUNDARY_ROWS)
    if case.weighted:
        rows[pc.tiny_row(case.graph)] = "weights summing to 1e-12"
    got = _check_case(case, rows=rows).cpu().numpy()
    if case.weighted:
        zero_row = pc.edge_weights(case.graph)[1]
        assert np.isfinite(got[zero_row]).all()
        if case.mode == "single":
            assert (got[zero_row] == 0.0).all()
    if case.mode == "single" and case.order == 1:
        # One step of `single` is one rounding: products of two float32 are exact in float64 and the float64 sums of
        # kernel and reference differ by ~1e-16 relative, so the stored float32 is within half an ulp of the reference,
        # |d| <= 2^-24 * |ref|.  (A float32 accumulator over 4096 neighbours misses this by an order of magnitude.)
        ref = pc.reference(case)
        half_ulp = 2.0 ** -24 * np.abs(ref) * (1 + 1e-6) + 1e-45
        for u, label in BOUNDARY_ROWS.items():
            assert (np.abs(got[u] - ref[u]) <= half_ulp[u]).all(), \
                f"row {u} ({label}): {np.abs(got[u] - ref[u]).max():.3e} is more than one rounding"
        assert (np.abs(got - ref) <= half_ulp).all()


def test_every_vector_width_and_lane_group():
    """F over every VEC in {1, 2, 4}, every lane group 2^0 .. 2^6, one and several trips of the column loop for each VEC,
    the exact fit G * VEC == F (256) and the datasets' own widths, on a graph with rows on both sides of kLongRow."""
    from grand_plus_amd import Graph
    indptr, indices = pc.graph("widths")
    g = Graph(indptr, indices, 0)
    vec_trips, groups = set(), set()
    for case in pc.WIDTH_CASES:
        vec = pc.vec_width(case.F)
        log2g = pc.lane_group_log2(case.F, vec)
        trips = -(-case.F // ((1 << log2g) * vec))
        assert vec * (1 << log2g) >= case.F or log2g == 6
        vec_trips.add((vec, min(trips, 2)))
        groups.add(log2g)
        rows = {u: f"degree {d}, F {case.F} (VEC {vec}, G {1 << log2g}, {trips} trips)" for u, d in enumerate((4097, 4400, 4096))}
        _check_case(case, g=g, rows=rows)
    g.close()
    assert vec_trips == {(v, t) for v in (1, 2, 4) for t in (1, 2)}, vec_trips
    assert groups == set(range(7)), groups
    assert 256 in pc.WIDTHS and pc.column_trips(256) == 1 and pc.vec_width(256) << pc.lane_group_log2(256, 4) == 256


def test_long_kernel_grid_stride():
    """180 long rows x 23 slabs of 64 columns (F = 1433, VEC 1) = 4140 work items for a grid capped at 4096: the first
    44 workgroups take a second item, through the `part` array a second time."""
    case = pc.LONG_STRIDE_CASE
    n_long = int((np.diff(pc.graph(case.graph)[0]) > pc.K_LONG_ROW).sum())
    slabs = pc.feature_slabs(case.F)
    assert (n_long, slabs) == (180, 23) and n_long * slabs == 4140 > pc.LONG_GRID_CAP
    _check_case(case, rows={0: "first long row", 43: "long row 43", 179: "last long row"})


def test_main_kernel_grid_stride():
    """40 000 rows at 4 rows per workgroup (F = 260: G = 64) = 10 000 row blocks for a grid capped at 8192."""
    case = pc.MAIN_STRIDE_CASE
    n = len(pc.graph(case.graph)[0]) - 1
    assert pc.rows_per_block(case.F) == 4 and -(-n // pc.rows_per_block(case.F)) > pc.MAIN_GRID_CAP
    _check_case(case, rows={n - 1: "last row", pc.MAIN_GRID_CAP * 4 + 1: "first row of the second pass"})


def test_results_are_bitwise_reproducible():
    """The long-row list is filled through an atomicAdd, so its order varies; every row is still reduced in a fixed order."""
    import torch
    from grand_plus_amd import Graph
    indptr, indices, _, _ = pc.inputs(pc.REPEAT_CASE)
    g = Graph(indptr, indices, 0)
    a = _check_case(pc.REPEAT_CASE, g=g)
    b = _check_case(pc.REPEAT_CASE, g=g)
    c = _check_case(pc.REPEAT_CASE, g=Graph(indptr, indices, 0))
    assert a.data_ptr() != b.data_ptr()
    assert torch.equal(a, b), f"{int((a != b).sum())} elements differ between two calls on one handle"
    assert torch.equal(a, c), f"{int((a != c).sum())} elements differ on a fresh handle"


def test_out_argument_side_stream_and_inputs_left_intact():
    import torch
    from grand_plus_amd import Graph
    case = pc.REPEAT_CASE
    indptr, indices, w, X = pc.inputs(case)
    g = Graph(indptr, indices, 0)
    x, dw = torch.tensor(X).cuda(), torch.tensor(w).cuda()
    x0, w0 = x.clone(), dw.clone()
    want = g.propagate_features(x, case.mode, case.order, case.alpha, edge_weight=dw)          # default stream
    out = torch.full_like(x, float("nan"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = g.propagate_features(x, case.mode, case.order, case.alpha, edge_weight=dw, out=out)
    side.synchronize()
    assert got is out
    assert torch.equal(out, want)
    assert torch.equal(x, x0) and torch.equal(dw, w0)
    _assert_close(out.cpu().numpy(), pc.reference(case), BOUNDARY_ROWS)
    # the same through _check's own out / stream parameters, and with the stream handed over explicitly
    out2 = torch.full_like(x, float("nan"))
    assert _check_case(case, g=g, out=out2, stream=side) is out2 and torch.equal(out2, want)
    out3 = torch.full_like(x, float("nan"))
    side.wait_stream(torch.cuda.current_stream())
    g.propagate_features(x, case.mode, case.order, case.alpha, edge_weight=dw, out=out3, stream=side.cuda_stream)
    side.synchronize()
    assert torch.equal(out3, want)


def test_alpha_at_zero_and_one_and_where_it_is_ignored():
    import torch
    from grand_plus_amd import Graph
    indptr, indices = pc.graph("hub")
    g = Graph(indptr, indices, 0)
    res = {c: _check_case(c, g=g) for c in pc.ALPHA_CASES}
    one, zero = pc.ALPHA_CASES[0], pc.ALPHA_CASES[1]
    assert (one.mode, one.alpha, zero.mode, zero.alpha) == ("ppr", 1.0, "ppr", 0.0)
    x = torch.tensor(pc.inputs(one)[3]).cuda()
    assert torch.equal(res[one], x)                                      # alpha = 1: nothing propagates, out = X exactly
    assert not torch.isnan(res[zero]).any() and torch.equal(res[zero], torch.zeros_like(x))
    for mode in ("avg", "single"):                                       # alpha is only read in ppr mode
        a, b = (res[c] for c in pc.ALPHA_CASES if c.mode == mode)
        assert torch.equal(a, b), mode


def _gfpush_rows(g, d_seeds, r, kernel):
    g.set_option("kernel", kernel)
    g.reset_stats()
    row, col, val, filled = g.gfpush_device(d_seeds, r.coef(), r.rmax, r.top_k)
    st = g.stats()
    assert st["kernel"] == kernel and st["failed_rows"] == 0
    f = filled.cpu().numpy()
    keep = (np.arange(r.top_k)[None, :] < f[:, None]).reshape(-1)
    return (np.where(keep, row.cpu().numpy(), 0), np.where(keep, col.cpu().numpy(), 0), np.where(keep, val.cpu().numpy(), 0.0))


def test_propagate_and_gfpush_share_one_handle_in_either_order():
    """propagate_features packs degrees into the handle's column words; the sketch kernel later builds its self-addressed
    CSR from them, the general kernel reads them.  One Graph: propagate, GFPush under each kernel (rows against the CPU
    oracle), propagate again -- bitwise the same.  A second Graph: GFPush first, then propagate."""
    import torch
    from grand_plus_amd import Graph, synth
    from grand_plus_amd.parity import compare_rows
    from grand_plus_amd.recipes import RECIPES
    from oracle import pyoracle
    case = pc.HANDLE_CASE
    indptr, indices, _, _ = pc.inputs(case)
    r = RECIPES[("mag", "ppr")]                                          # as test_gpu_sketch.py runs it on this graph
    seeds = synth.seeds(len(indptr) - 1, 512)
    d_seeds = torch.from_numpy(seeds).cuda()
    erow, ecol, eval_, est = pyoracle.gfpush(indptr, indices, seeds, r.coef(), r.rmax, r.top_k, want_next=True)

    def rows_are_the_oracles(g, kernel, label):
        rep = compare_rows(seeds, r.top_k, _gfpush_rows(g, d_seeds, r, kernel), (erow, ecol, eval_), next_value=est["next_value"])
        assert rep.ok, f"{label}, kernel {kernel}:\n" + "\n".join(rep.messages)

    g = Graph(indptr, indices, 0)
    a = _check_case(case, g=g)
    for kernel in (2, 1):
        rows_are_the_oracles(g, kernel, "after propagate_features")
    b = _check_case(case, g=g)
    assert torch.equal(a, b)
    g.close()

    g = Graph(indptr, indices, 0)
    for kernel in (2, 1):
        rows_are_the_oracles(g, kernel, "before propagate_features")
    c = _check_case(case, g=g)
    assert torch.equal(a, c)
    g.close()


def test_argument_errors_are_raised_before_anything_runs():
    import torch
    from grand_plus_amd import Graph
    indptr, indices = pc.graph("hub")
    n, F = len(indptr) - 1, 8
    g = Graph(indptr, indices, 0)
    x = torch.ones((n, F), device="cuda")
    out = torch.full_like(x, float("nan"))
    for alpha in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            g.propagate_features(x, "ppr", 2, alpha, out=out)
    with pytest.raises(ValueError):
        g.propagate_features(x, "ppr", -1, out=out)
    with pytest.raises(ValueError):
        g.propagate_features(torch.zeros((n, 0), device="cuda"), "ppr", 2)
    w = torch.ones(len(indices), device="cuda")
    with pytest.raises(TypeError):
        g.propagate_features(x, "ppr", 2, edge_weight=w[:-1].contiguous(), out=out)
    with pytest.raises(TypeError):
        g.propagate_features(x, "ppr", 2, edge_weight=w.double(), out=out)
    for bad in (torch.empty((n - 1, F), device="cuda"),                 # too few rows
                torch.empty((n, F), device="cuda", dtype=torch.float64),
                torch.empty((F, n), device="cuda").t(),                 # the right shape, transposed strides
                torch.empty((n, F))):                                   # on the CPU
        with pytest.raises(TypeError, match="out must be"):
            g.propagate_features(x, "ppr", 2, out=bad)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()                                        # no refused call wrote a result
    g.close()
