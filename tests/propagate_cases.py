"""Graphs, cases, the fp32-storage emulation and the tolerance shared by the propagate_features tests
(tests/test_gpu_propagate.py on the GPU, tests/test_host_propagate.py on the CPU).  The reference
itself is oracle/predict_ref.py."""
import functools
from collections import namedtuple

import numpy as np

K_LONG_ROW = 4096          # propagate.hip's kLongRow: rows with more neighbours go to spmm_long_kernel
MAIN_GRID_CAP = 256 * 32   # ... and the caps of the two kernels' grids
LONG_GRID_CAP = 4096


def tolerance(ref):
    """The module's bound per element: |d| <= 2e-6*|ref| + 1e-6*max|ref| (fp32 storage rounded once per step
    against the float64 restatement, up to 20 steps)."""
    ref = np.abs(np.asarray(ref, dtype=np.float64))
    return 2e-6 * ref + 1e-6 * ref.max()


# -- the launch geometry of gp_common.hpp, restated ------------------------------------------------------
def vec_width(F):
    return 4 if F % 4 == 0 else 2 if F % 2 == 0 else 1


def lane_group_log2(F, vec):
    log2g = 0
    while log2g < 6 and (1 << log2g) * vec < F:
        log2g += 1
    return log2g


def column_trips(F):
    """Trips of spmm_kernel's `for (f = gl*VEC; f < F; f += G*VEC)` loop."""
    vec = vec_width(F)
    span = (1 << lane_group_log2(F, vec)) * vec
    return -(-F // span)


def rows_per_block(F):
    return 4 * (64 >> lane_group_log2(F, vec_width(F)))


def feature_slabs(F):
    return -(-F // (64 * vec_width(F)))


# -- graphs ------------------------------------------------------------------------------------------------
def hub_graph(n, hub_degrees, seed, max_small=12):
    """(indptr, indices) int32: row u < len(hub_degrees) has exactly hub_degrees[u] distinct sorted neighbours;
    of the other rows, every one with u % 7 == 0 is dangling and the rest have 1 .. max_small neighbours."""
    rng = np.random.default_rng(seed)
    rows = []
    for u in range(n):
        if u < len(hub_degrees):
            deg = int(hub_degrees[u])
        elif u % 7 == 0:
            deg = 0
        else:
            deg = int(rng.integers(1, max_small + 1))
        rows.append(np.sort(rng.choice(n, size=deg, replace=False)))
    indptr = np.zeros(n + 1, np.int32)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    return indptr, np.concatenate(rows).astype(np.int32)


# degree: why
HUB_DEGREES = (4096,       # the last degree the main kernel takes
               4097,       # the first degree the long kernel takes
               4227,       # 4096 + 128 + 3: the long kernel's tail loop
               5999,       # the largest degree that fits
               4104,       # a further long row
               8, 16, 17, 9, 1)      # batch-of-8 edges of the main kernel
N_BOUNDARY_ROWS = 5        # rows 0..4 of the standard hub graph are asserted by name

GRAPHS = {
    "hub": dict(n=6000, hub_degrees=HUB_DEGREES, seed=1),                       # the standard hub graph
    "widths": dict(n=4500, hub_degrees=(4097, 4400, 4096), seed=5),
    "long_stride": dict(n=6000, hub_degrees=(4097,) * 180, seed=3),             # n_long * slabs > the long grid
    "main_stride": dict(n=40000, hub_degrees=(), seed=4, max_small=8),          # more row blocks than the main grid
}
SKETCH_GRAPH = "sketch"    # synth "small": the graph tests/test_gpu_sketch.py runs the sketch kernel on


@functools.lru_cache(maxsize=None)
def graph(name):
    if name == SKETCH_GRAPH:
        from grand_plus_amd import synth
        indptr, indices = synth.shape_csr("small")
    else:
        indptr, indices = hub_graph(**GRAPHS[name])
    for a in (indptr, indices):
        a.setflags(write=False)
    return indptr, indices


@functools.lru_cache(maxsize=None)
def edge_weights(name):
    """(float32 [nnz] drawn from uniform(0.5, 2.0), zero_row): the stored values of a weighted adjacency; the weights
    of one short row are all 0.0, so its row sum is 0, max(deg, 1e-12) takes its other branch and the row must come
    out 0, not NaN.  The next short row (`tiny_row`) has two weights of 5e-13 and zeros: its row sum is the 1e-12 of
    max(deg, 1e-12) itself, where deg + 1e-12 would halve the row."""
    indptr, indices = graph(name)
    w = np.random.default_rng(GRAPHS[name]["seed"] + 100).uniform(0.5, 2.0, size=len(indices)).astype(np.float32)
    deg = np.diff(indptr)
    n_hubs = len(GRAPHS[name]["hub_degrees"])
    zero_row = n_hubs + int(np.flatnonzero((deg[n_hubs:] >= 2) & (deg[n_hubs:] <= 12))[0])
    w[indptr[zero_row]:indptr[zero_row + 1]] = 0.0
    tiny = tiny_row(name)
    w[indptr[tiny]:indptr[tiny + 1]] = 0.0
    w[indptr[tiny]:indptr[tiny] + 2] = TINY_WEIGHT
    w.setflags(write=False)
    return w, zero_row


TINY_WEIGHT = np.float32(5e-13)


def tiny_row(name):
    """The second row of 2 .. 12 neighbours after the hubs: the first is the zero row."""
    deg = np.diff(graph(name)[0])
    n_hubs = len(GRAPHS[name]["hub_degrees"])
    return n_hubs + int(np.flatnonzero((deg[n_hubs:] >= 2) & (deg[n_hubs:] <= 12))[1])


# -- cases: every (graph, F, mode, order, alpha, weights) the GPU tests run ----------------------------------
Case = namedtuple("Case", "graph F mode order alpha weighted")
Case.__str__ = lambda c: f"{c.graph}-F{c.F}-{c.mode}-o{c.order}-a{c.alpha}-{'w' if c.weighted else 'u'}"

MODES = ("ppr", "avg", "single")
HUB_CASES = [Case("hub", F, mode, order, alpha, weighted) for F in (12, 65) for mode in MODES
             for weighted in (False, True) for order, alpha in ((1, 0.2), (5, 0.3))] + \
            [Case("hub", 65, "avg", 20, 0.2, True)]
WIDTHS = (2, 3, 4, 6, 8, 12, 16, 65, 66, 128, 252, 256, 258, 260, 500, 602, 1433,
          9, 10, 20, 36)   # ... lane groups of 8 and 16 (log2g 3 and 4), which none of the widths above has
WIDTH_CASES = [Case("widths", F, "ppr", 2, 0.2, False) for F in WIDTHS]
LONG_STRIDE_CASE = Case("long_stride", 1433, "ppr", 2, 0.2, False)
MAIN_STRIDE_CASE = Case("main_stride", 260, "avg", 3, 0.2, False)
REPEAT_CASE = Case("hub", 65, "ppr", 5, 0.3, True)                 # determinism; out= and stream
ALPHA_CASES = [Case("hub", 12, "ppr", 3, 1.0, False), Case("hub", 12, "ppr", 3, 0.0, False)] + \
              [Case("hub", 12, mode, 3, alpha, False) for mode in ("avg", "single") for alpha in (0.2, 0.9)]
HANDLE_CASE = Case(SKETCH_GRAPH, 32, "ppr", 4, 0.2, False)
ALL_CASES = list(dict.fromkeys(HUB_CASES + WIDTH_CASES + [LONG_STRIDE_CASE, MAIN_STRIDE_CASE, REPEAT_CASE] +
                               ALPHA_CASES + [HANDLE_CASE]))


@functools.lru_cache(maxsize=4)
def features(n, F):
    X = np.random.default_rng(F).standard_normal((n, F)).astype(np.float32)
    X.setflags(write=False)
    return X


def inputs(case):
    """(indptr, indices, weights float32 or None, X float32 [n, F]) of a case; shared and read-only."""
    indptr, indices = graph(case.graph)
    w = edge_weights(case.graph)[0] if case.weighted else None
    return indptr, indices, w, features(len(indptr) - 1, case.F)


def _adjacency(indptr, indices, weights):
    import scipy.sparse as sp
    n = len(indptr) - 1
    data = np.ones(len(indices)) if weights is None else np.asarray(weights, dtype=np.float64)
    return sp.csr_matrix((data, indices, indptr), shape=(n, n))


@functools.lru_cache(maxsize=8)
def reference(case):
    """oracle.predict_ref.propagate_ref of a case (float64), computed once and read-only."""
    from oracle.predict_ref import propagate_ref
    indptr, indices, w, X = inputs(case)
    ref = propagate_ref(_adjacency(indptr, indices, w), X, case.mode, case.order, case.alpha)
    ref.setflags(write=False)
    return ref


# -- the reference written out, and one deliberate mistake (tests/test_host_mutants.py) -----------------------------
MUTANTS = ("deg_plus_eps", "alpha_on_every_term", "avg_over_n", "single_returns_sum", "alpha_missing_on_x0")


def propagate_manual64(case, mut=None):
    """oracle.predict_ref.propagate_ref of a case from explicit formulas (mut None), or with one of MUTANTS built in."""
    indptr, indices, w, X = inputs(case)
    adj = _adjacency(indptr, indices, w)
    deg = np.asarray(adj.sum(1)).reshape(-1)
    inv = 1.0 / (deg + 1e-12) if mut == "deg_plus_eps" else 1.0 / np.maximum(deg, 1e-12)
    ppr = case.mode == "ppr"
    step = ((1.0 - case.alpha) if ppr else 1.0) * inv
    if ppr and mut == "alpha_on_every_term":
        step = case.alpha * step
    x = np.asarray(X, dtype=np.float64)
    if ppr and mut != "alpha_missing_on_x0":
        x = case.alpha * x
    total = x.copy()
    for _ in range(case.order):
        x = step[:, None] * adj.dot(x)
        total += x
    if case.mode == "single":
        return total if mut == "single_returns_sum" else x
    if case.mode == "avg":
        with np.errstate(divide="ignore", invalid="ignore"):
            return total / (case.order if mut == "avg_over_n" else case.order + 1)
    return total


def share(got, ref):
    """max |got - ref| / tolerance; a non-finite entry counts as infinite."""
    d, tol = np.abs(got - ref), tolerance(ref)
    if not np.isfinite(d).all() or (d > 0)[tol == 0].any():
        return float("inf")
    return float((d[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0


def emulate_fp32_storage(indptr, indices, weights, X, mode, order, alpha):
    """The arithmetic contract of propagate.hip in numpy: sums in float64 over float32 weights and float32 state, a
    float64 scale, the state rounded to float32 once per step, the running sum added in float32 and, for avg, the
    final factor the float32 1/(order+1).  Not a second reference: it shows that `tolerance` is met by the storage
    format alone."""
    adj = _adjacency(indptr, indices, None if weights is None else np.asarray(weights, dtype=np.float32))
    deg = np.asarray(adj.sum(1)).reshape(-1)
    scale = ((1.0 - alpha) if mode == "ppr" else 1.0) / np.maximum(deg, 1e-12)
    x = np.asarray(X, dtype=np.float32)
    if mode == "ppr":
        x = np.float32(alpha) * x
    total = x.copy()
    for _ in range(order):
        x = (scale[:, None] * adj.dot(x.astype(np.float64))).astype(np.float32)
        if mode != "single":
            total = total + x
    if mode == "single":
        return x
    if mode == "avg":
        total = total * (np.float32(1.0) / np.float32(order + 1))
    assert total.dtype == np.float32
    return total
