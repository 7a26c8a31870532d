"""CPU proof that the tolerance of tests/test_gpu_propagate.py is met by fp32 storage alone: for every case the GPU
tests run, the numpy statement of the kernel's arithmetic contract (propagate_cases.emulate_fp32_storage) stays
inside propagate_cases.tolerance of the float64 restatement (oracle/predict_ref.py).  A GPU result outside the
bound is therefore a kernel finding.  Measured here: worst |d| / tol 0.08 (avg, order 20), below 0.07 elsewhere.
Also: what the graph builder promises, and the launch geometry the case list is chosen for."""
import numpy as np
import pytest

import propagate_cases as pc


@pytest.mark.parametrize("case", pc.ALL_CASES, ids=str)
def test_fp32_storage_alone_meets_the_tolerance(case):
    if case.F == 1433 and case.order > 1:
        case = case._replace(order=1)                  # the widest products once, to keep this suite quick
    indptr, indices, w, X = pc.inputs(case)
    ref = pc.reference(case)
    emu = pc.emulate_fp32_storage(indptr, indices, w, X, case.mode, case.order, case.alpha)
    assert emu.dtype == np.float32 and emu.shape == ref.shape and np.isfinite(emu).all()
    ratio = (np.abs(emu - ref) / pc.tolerance(ref)).max() if np.abs(ref).max() > 0 else np.abs(emu).max()
    print(f"[emulation] {case}: worst |d| / tol {ratio:.3f}")
    assert ratio <= 1.0, f"{case}: fp32 storage alone is {ratio:.2f} x the tolerance"


@pytest.mark.parametrize("name", sorted(pc.GRAPHS))
def test_hub_graph_is_what_it_promises(name):
    spec = pc.GRAPHS[name]
    indptr, indices = pc.graph(name)
    n, hubs = spec["n"], spec["hub_degrees"]
    assert indptr.dtype == np.int32 and indices.dtype == np.int32
    assert len(indptr) == n + 1 and indptr[0] == 0 and indptr[-1] == len(indices)
    deg = np.diff(indptr)
    assert deg[:len(hubs)].tolist() == list(hubs)
    rest = np.arange(len(hubs), n)
    dangling = rest[rest % 7 == 0]
    others = rest[rest % 7 != 0]
    assert len(dangling) > 0 and (deg[dangling] == 0).all()
    assert deg[others].min() == 1 and deg[others].max() == spec.get("max_small", 12)
    assert indices.min() >= 0 and indices.max() < n
    inner = np.ones(len(indices), bool)
    inner[indptr[:-1][deg > 0]] = False                # the first neighbour of every row has no predecessor in it
    assert (np.diff(indices.astype(np.int64), prepend=-1)[inner] > 0).all(), "a row is not sorted and distinct"


def test_weighted_variant_has_one_short_row_of_zero_weights():
    """... and, since the audit of DESIGN §7q, one short row at the epsilon's scale."""
    indptr, indices = pc.graph("hub")
    w, zero_row = pc.edge_weights("hub")
    assert w.dtype == np.float32 and len(w) == len(indices)
    assert zero_row >= len(pc.HUB_DEGREES) and 2 <= indptr[zero_row + 1] - indptr[zero_row] <= 12
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    assert (w[rows == zero_row] == 0.0).all()
    tiny = pc.tiny_row("hub")                          # ... and one whose weights sum to the 1e-12 of max(deg, 1e-12)
    assert tiny > zero_row and 2 <= indptr[tiny + 1] - indptr[tiny] <= 12
    assert w[rows == tiny][:2].tolist() == [pc.TINY_WEIGHT] * 2 and (w[rows == tiny][2:] == 0.0).all()
    assert abs(float(w[rows == tiny].astype(np.float64).sum()) - 1e-12) < 1e-18
    other = (rows != zero_row) & (rows != tiny)
    assert w[other].min() >= 0.5 and w[other].max() <= 2.0
    for mode in pc.MODES:                              # scale = numer / 1e-12 times a sum of 0: 0, never NaN
        ref = pc.reference(pc.Case("hub", 12, mode, 1, 0.2, True))
        assert np.isfinite(ref).all()
        if mode == "single":
            assert (ref[zero_row] == 0.0).all()


def test_cases_reach_the_paths_they_are_chosen_for():
    """The geometry of gp_common.hpp / propagate.hip, restated: the standard hub graph sits on both sides of kLongRow
    and in the long kernel's tail loop; the two grid-stride cases exceed the grids' caps."""
    deg = np.diff(pc.graph("hub")[0])
    assert deg[0] == pc.K_LONG_ROW and deg[1] == pc.K_LONG_ROW + 1
    assert (deg[2] - pc.K_LONG_ROW) % 128 == 3 and deg[3] == pc.GRAPHS["hub"]["n"] - 1
    assert (deg[:pc.N_BOUNDARY_ROWS] >= pc.K_LONG_ROW).all() and deg[pc.N_BOUNDARY_ROWS:].max() < pc.K_LONG_ROW
    c = pc.LONG_STRIDE_CASE
    n_long = int((np.diff(pc.graph(c.graph)[0]) > pc.K_LONG_ROW).sum())
    assert (n_long, pc.feature_slabs(c.F)) == (180, 23) and n_long * pc.feature_slabs(c.F) > pc.LONG_GRID_CAP
    c = pc.MAIN_STRIDE_CASE
    assert -(-pc.GRAPHS[c.graph]["n"] // pc.rows_per_block(c.F)) > pc.MAIN_GRID_CAP
    seen = {(pc.vec_width(F), min(pc.column_trips(F), 2)) for F in pc.WIDTHS}
    assert seen == {(v, t) for v in (1, 2, 4) for t in (1, 2)}
    assert {pc.lane_group_log2(F, pc.vec_width(F)) for F in pc.WIDTHS} == set(range(7))
