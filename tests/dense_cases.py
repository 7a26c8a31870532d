"""A numpy mirror of the dense-LDS GFPush kernel (grand_plus_amd/csrc/gfpush_dense.hpp, option kernel = 3) and the mistakes it
is most likely to hold.

dense_rows() restates the kernel as it is built: three dense fp64 arrays indexed by node id that SURVIVE from row to row (cur,
next, reserve) and a touched mark per node, a level sweep over every node with cur != 0, the reference's push test
r >= rmax * (double)deg with deg the indptr difference (precompute/graph.h:94), dangling nodes returning to the seed untested
(graph.h:91-93), and a strict select over the dense reserve among the values > 0 by (value desc, column asc).  MUTANTS lists
deliberate mistakes; MOVED_BY names, per mistake, a graph of the existing case modules that it moves (tests/test_host_dense.py
audits that, and that the unmutated mirror equals the dict walk of tests/push_boundary_cases.py on every case)."""
import numpy as np

import push_boundary_cases as pb
import select_boundary_cases as sb

DENSE_MAX_NODES = 6720                 # kDenseMaxNodes of gfpush_plan.hpp (tests/test_host_dense.py holds the two equal)

MUTANTS = ("gt", "deg_saturated", "dangling_tested", "stale_reserve", "select_value_only")

# mistake -> (module, case name, keyword arguments of run_case) of a case it must move
MOVED_BY = {
    "gt": ("pb", "l1_1e-4", {}),
    "deg_saturated": ("pb", "saturation", {"deg_sat": 3}),
    "dangling_tested": ("pb", "dangling", {}),
    "stale_reserve": ("pb", "saturation", {}),
    "select_value_only": ("sb", "tie_g2", {}),
}


class DenseState:
    """What a workgroup keeps in LDS between rows."""

    def __init__(self, n):
        self.cur, self.nxt, self.reserve = np.zeros(n), np.zeros(n), np.zeros(n)
        self.mark = np.zeros(n, bool)


def dense_row(state, indptr, indices, seed, coef, rmax, K, mut=None, deg_sat=0):
    """One row on the state the previous row left.  Returns ([(column, value)] in slot order, counters)."""
    assert mut is None or mut in MUTANTS, mut
    n_coef = len(coef)
    pushes = edges = frontier = 0
    state.cur[seed] = 1.0                                              # graph.h:81
    for lvl in range(n_coef):
        last = lvl == n_coef - 1
        front = np.flatnonzero(state.cur != 0.0)
        if len(front) == 0:
            break
        frontier += len(front)
        state.mark[front] = True
        for v in front.tolist():
            r = float(state.cur[v])
            state.reserve[v] = state.reserve[v] + float(coef[lvl]) * r    # graph.h:90 / :109
            state.cur[v] = 0.0
            if last:
                continue
            lo, hi = int(indptr[v]), int(indptr[v + 1])
            deg = hi - lo
            if deg == 0:                                               # graph.h:91-93
                if mut == "dangling_tested" and not r >= rmax:
                    continue
                state.nxt[seed] += r
                continue
            d_test = min(deg, deg_sat) if mut == "deg_saturated" and deg_sat else deg
            taken = r > rmax * float(d_test) if mut == "gt" else r >= rmax * float(d_test)       # graph.h:94
            if taken:
                share = r / float(deg)                                 # graph.h:95
                for j in range(lo, hi):                                # graph.h:96-99: once per stored entry
                    state.nxt[int(indices[j])] += share
                pushes += 1
                edges += deg
        state.cur, state.nxt = state.nxt, state.cur
    support = int(state.mark.sum())
    cols = np.flatnonzero(state.reserve > 0.0)                         # graph.h:121
    vals = state.reserve[cols]
    if mut == "select_value_only":
        order = np.lexsort((-cols, -vals))                             # ties in whatever order: here the larger column first
    else:
        order = np.lexsort((cols, -vals))                              # (value desc, column asc)
    row = [(int(cols[i]), float(vals[i])) for i in order[:K]]
    if mut != "stale_reserve":                                         # the state the next row assumes
        state.reserve[state.mark] = 0.0
    state.mark[:] = False
    state.cur[:] = 0.0
    state.nxt[:] = 0.0
    return row, (pushes, edges, len(row), support, frontier)


def dense_rows(indptr, indices, seeds, coef, rmax, K, mut=None, deg_sat=0):
    """Every seed in order on one workgroup's state.  Returns (rows, summed counters (pushes, edges, filled, support, frontier))."""
    state = DenseState(len(indptr) - 1)
    rows, total = [], np.zeros(5, np.int64)
    for s in seeds:
        row, ctr = dense_row(state, indptr, indices, int(s), coef, rmax, K, mut, deg_sat)
        rows.append(row)
        total += ctr
    return rows, tuple(int(x) for x in total)


def case_inputs(module, name):
    """(indptr, indices, seeds, coef, rmax, K) of a case of push_boundary_cases ("pb": under a K above every support) or of
    select_boundary_cases ("sb": compacted, under its first K)."""
    if module == "pb":
        case = pb.cases()[name]
        return case.indptr, case.indices, case.seeds, case.coef, case.rmax, case.full_k()
    case = sb.cases()[name]
    indptr, indices, seeds, _ = case.compact(limit=1 << 30)
    return indptr, indices, seeds, case.coef, case.rmax, case.ks[0]


def run_case(module, name, mut=None, deg_sat=0):
    indptr, indices, seeds, coef, rmax, K = case_inputs(module, name)
    return dense_rows(indptr, indices, seeds, coef, rmax, K, mut, deg_sat)


def reference_rows(module, name):
    """The same case by the dict walk of push_boundary_cases and the strict select of select_boundary_cases."""
    indptr, indices, seeds, coef, rmax, K = case_inputs(module, name)
    walks = [pb.push_walk64(indptr, indices, s, coef, rmax) for s in seeds]
    rows = [sb.select_exact(w.reserve, K) for w in walks]
    ctr = (sum(w.pushes for w in walks), sum(w.edges for w in walks), sum(len(r) for r in rows),
           sum(len(w.reserve) for w in walks), sum(w.frontier_sum for w in walks))
    return rows, ctr
