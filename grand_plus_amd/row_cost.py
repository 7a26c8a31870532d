"""The row cost and cost class behind option "row_order", restated in numpy (csrc/gfpush_kernels.hpp: row_cost_kernel).

The first launch of a GFPush call hands out its rows heaviest first.  A row's cost is the edge count of its levels 1 and 2,
which the seed's own columns give (graph.h:94 is the push test, the residue reaching a neighbour of the seed is 1/d0):

    c = 0                                 the seed is invalid (< 0 or >= n_nodes), dangling, or fails the push test itself
    c = d0 + floor(d0 * sum / n)          sum = SUM over the first n = min(d0, COST_COLS) columns u of
                                                [1/d0 >= rmax * deg(u)] * deg(u),   deg(u) = min(degree of u, deg_sat)

(n = d0 for all but hub seeds, where the sum over the columns read is scaled to the whole row), and its class is
min(31, ilog2(c + 1)).  `deg_sat` is where the packed degree field of the device's column words saturates: a saturated degree
counts as deg_sat, in the test and in the sum.  tests/test_host_row_order.py pins this definition on a hand-made graph,
tests/test_gpu_row_order.py holds the device's order against it, tools/sim/run_row_order_sim.py prices it.
"""
from __future__ import annotations

import numpy as np

COST_COLS = 256          # kCostCols
N_CLASSES = 32


def row_costs(indptr, indices, seeds, rmax, deg_sat, cols=COST_COLS):
    """int64[len(seeds)]: the cost of every row (exact integer arithmetic, the push test in float64 as the kernel has it)."""
    indptr = np.asarray(indptr, np.int64)
    indices = np.asarray(indices, np.int64)
    n = len(indptr) - 1
    deg = np.minimum(np.diff(indptr), int(deg_sat))
    out = np.zeros(len(seeds), np.int64)
    rmax = np.float64(rmax)
    for i, s in enumerate(np.asarray(seeds, np.int64)):
        if s < 0 or s >= n:
            continue
        d0 = int(indptr[s + 1] - indptr[s])
        if d0 == 0 or not (np.float64(1.0) >= rmax * np.float64(d0)):
            continue
        n_read = min(d0, cols)
        dg = deg[indices[indptr[s]:indptr[s] + n_read]]
        share = np.float64(1.0) / np.float64(d0)
        total = int(dg[share >= rmax * dg.astype(np.float64)].sum())
        out[i] = d0 + (d0 * total) // n_read
    return out


def cost_class(cost):
    """min(31, ilog2(c + 1)) of every cost."""
    return np.array([min(N_CLASSES - 1, (int(c) + 1).bit_length() - 1) for c in np.asarray(cost, np.int64).reshape(-1)], np.int64)


def order_by_class(classes):
    """A row order the device may produce: classes descending (stable inside a class; the device's order inside a class is free)."""
    return np.argsort(-np.asarray(classes, np.int64), kind="stable")
