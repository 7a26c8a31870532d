"""GFPush's push test `r >= rmax * deg` (graph.h:94) held at its threshold: case graphs, a float64 walk, a filter mirror.

Three things live here, all plain Python / numpy on the CPU:

  * push_walk64: oracle/gfpush_oracle.cpp restated line for line on dicts, returning the reserve map, the counters and every
    decision (level, node, deg, r, rmax * deg, taken).  `level` is the oracle's loop index at which the node is drained, which
    is its distance from the seed on these graphs: 0 for the seed, 1 for the seed's neighbours.  `mut` swaps in one
    deliberate mistake (MUTANTS); mut=None equals oracle.pyoracle.gfpush (tests/test_host_push_boundary.py).
  * filter_candidates: the sketch kernel's fp32 candidate test alone (phase_sk_filter: (float)cell >= (float)dq * thr with
    cell = sum of ceil(share * 2^31) over the edges into the node), on per-node cells or on the hashed cells of
    collision_cases' mirror of gfpush_hash.hpp, with its own mistakes (FILTER_MUTANTS).
  * cases(): small graphs built constructively (no search at import) that put a node on the threshold bit for bit, one ulp
    to either side of it, or one edge beyond it, at every level and path of both kernels.  GPU_CASES is the list
    tests/test_gpu_push_boundary.py parametrises over and tests/test_host_push_boundary.py audits.

How the degrees were found: for rmax = 1/N, tuples (d0, ..., dl) with d0 * ... * dl = N are mathematically ties,
((1/d0)/d1)/... against rmax * dl; float64 puts each of them bit-equal ("eq"), one ulp above ("above": pushes) or one
ulp below ("below": does not push).  All tuples at 1e-4 and 1e-5 are "eq"; 1e-6 has "above" tuples from depth 2 on;
1/12000 has "eq" and "above"; 1/4800 has "eq" and "below".  The host test asserts the class each case claims.
"""
from __future__ import annotations

import functools
import math
from collections import namedtuple

import numpy as np

import collision_cases as cc

MUTANTS = ("gt", "cmp_f32", "prod_f32", "rmax_f32", "quotient", "deg_packed", "seed_untested", "dangling_tested",
           "unpushed_carried")
FILTER_MUTANTS = ("thr_up_no_margin", "thr_nearest_no_margin", "share_floor_no_margin")

Walk = namedtuple("Walk", "reserve pushes edges dangling decisions frontier_sum returns")
Decision = namedtuple("Decision", "level node deg r thr taken")


def _f32(x):
    return float(np.float32(x))


def push_walk64(indptr, indices, seed, coef, rmax, mut=None, deg_sat=0):
    """One row of oracle/gfpush_oracle.cpp.  deg_sat: the saturation value of the packed degree field, read by the
    `deg_packed` mistake alone (0: the field is never saturated)."""
    assert mut is None or mut in MUTANTS, mut
    n_coef = len(coef)
    res, rsv = {int(seed): 1.0}, {int(seed): 0.0}                      # graph.h:81-82
    pushes = edges = dangling = frontier = 0
    decisions, returns = [], []                                        # returns: (level, node, r) of every dangling return
    for lvl in range(n_coef - 1):                                      # graph.h:83
        nxt = {}
        c = float(coef[lvl])
        frontier += len(res)
        for u, r in res.items():                                       # graph.h:85-89
            rsv[u] = rsv.get(u, 0.0) + c * r                           # graph.h:90
            lo, hi = int(indptr[u]), int(indptr[u + 1])
            deg = hi - lo                                              # graph.h:43-45
            if deg == 0:                                               # graph.h:91-93
                if mut == "dangling_tested" and not r >= rmax:
                    continue
                nxt[int(seed)] = nxt.get(int(seed), 0.0) + r
                dangling += 1
                returns.append((lvl, u, r))
                continue
            thr = rmax * deg
            if mut == "gt":
                taken = r > thr
            elif mut == "cmp_f32":
                taken = _f32(r) >= _f32(thr)
            elif mut == "prod_f32":
                taken = r >= float(np.float32(rmax) * np.float32(deg))
            elif mut == "rmax_f32":
                taken = r >= _f32(rmax) * deg
            elif mut == "quotient":
                taken = r / deg >= rmax
            elif mut == "deg_packed":
                taken = r >= rmax * (min(deg, deg_sat) if deg_sat else deg)
            elif mut == "seed_untested":
                taken = r >= thr or (lvl == 0 and u == seed)
            else:
                taken = r >= thr                                       # graph.h:94
            decisions.append(Decision(lvl, u, deg, r, thr, taken))
            if taken:
                share = r / deg                                        # graph.h:95
                for j in range(lo, hi):                                # graph.h:96-99
                    v = int(indices[j])
                    nxt[v] = nxt.get(v, 0.0) + share
                pushes += 1
                edges += deg
            elif mut == "unpushed_carried":
                nxt[u] = nxt.get(u, 0.0) + r
        res = nxt                                                      # graph.h:102
    c = float(coef[n_coef - 1])
    frontier += len(res)
    for u, r in res.items():                                           # graph.h:104-110
        rsv[u] = rsv.get(u, 0.0) + c * r
    return Walk(rsv, pushes, edges, dangling, decisions, frontier, returns)


def walk_case(case, mut=None, deg_sat=0):
    """Every seed of a case: (list of Walk, total pushes, total edges)."""
    walks = [push_walk64(case.indptr, case.indices, s, case.coef, case.rmax, mut, deg_sat) for s in case.seeds]
    return walks, sum(w.pushes for w in walks), sum(w.edges for w in walks)


def ulps(a, b):
    """a - b in units of the last place (both positive doubles)."""
    return int(np.float64(a).view(np.int64)) - int(np.float64(b).view(np.int64))


# ------------------------------------------------------------------ how near real inputs come to the threshold

def near_threshold_counts(indptr, indices, seeds, coef, rmax, rel=2.0 ** -20):
    """Level-synchronous numpy walk of the same algorithm (sums by np.bincount: the order of the adds differs from the dict
    walk's in the last bits, which a window of 2^-20 does not see).  Returns (decisions, within rel of the threshold,
    bit-equal to it)."""
    indptr = np.asarray(indptr, np.int64)
    indices = np.asarray(indices, np.int64)
    n = len(indptr) - 1
    deg_all = np.diff(indptr)
    total = near = equal = 0
    for seed in seeds:
        nodes = np.array([int(seed)], np.int64)
        r = np.array([1.0])
        for _ in range(len(coef) - 1):
            deg = deg_all[nodes]
            live = deg > 0
            thr = rmax * deg.astype(np.float64)
            total += int(live.sum())
            near += int((live & (np.abs(r - thr) <= rel * thr)).sum())
            equal += int((live & (r == thr)).sum())
            push = live & (r >= thr)
            ret = float(r[~live].sum())
            pn, pr, pd = nodes[push], r[push], deg[push]
            if len(pn):
                starts = indptr[pn]
                offs = np.arange(int(pd.sum())) - np.repeat(np.cumsum(pd) - pd, pd)
                cols = indices[np.repeat(starts, pd) + offs]
                acc = np.bincount(cols, weights=np.repeat(pr / pd, pd), minlength=n)
            else:
                acc = np.zeros(n)
            if (~live).any():
                acc[int(seed)] += ret
                hit = acc > 0
                hit[int(seed)] = True
            else:
                hit = acc > 0
            nodes = np.flatnonzero(hit)
            r = acc[nodes]
            if len(nodes) == 0:
                break
    return total, near, equal


# ------------------------------------------------------------------ the sketch filter's arithmetic

def filter_threshold(rmax, mut=None):
    """kp.sk_thr_f of launch_sketch (gfpush.hip): rmax * 2^31 * (1 - 2^-10), rounded DOWN to float32."""
    assert mut is None or mut in FILTER_MUTANTS, mut
    if mut is None:
        x = rmax * 2147483648.0 * (1.0 - 1.0 / 1024.0)
        t = np.float32(x)
        while float(t) > x:
            t = np.nextafter(t, np.float32(0.0))
        return t
    x = rmax * 2147483648.0
    t = np.float32(x)
    if mut == "thr_up_no_margin":
        while float(t) < x:
            t = np.nextafter(t, np.float32(np.inf))
    elif mut == "share_floor_no_margin":
        while float(t) > x:
            t = np.nextafter(t, np.float32(0.0))
    return t


def filter_candidates(case, seed, mut=None, lg_mu=None, max_degree_bits=31):
    """Per level >= 1 of the true walk of `seed`: which frontier nodes the sketch filter keeps.

    Returns a list of (level, node, true_pusher, candidate).  lg_mu=None gives every node a cell of its own (the arithmetic
    alone); otherwise cells are the 2^lg_mu hashed ones of the kernel (sk_cell of the self-addressed key), where collisions
    can only add to a cell."""
    thr = filter_threshold(case.rmax, mut)
    fx = math.floor if mut == "share_floor_no_margin" else math.ceil
    indptr, indices = case.indptr, case.indices
    deg_all = np.diff(indptr)
    if lg_mu is None:
        cell_of = np.arange(len(deg_all))
        dq_all = deg_all
    else:
        _, _, a_sat, key = cc.acsr_layout(indptr, max_degree_bits)
        cell_of = (cc.sk_cell(key) >> np.uint64(32 - lg_mu)).astype(np.int64)
        dq_all = np.minimum(deg_all, a_sat)
    walk = push_walk64(indptr, indices, seed, case.coef, case.rmax)
    by_level = {}
    for d in walk.decisions:
        by_level.setdefault(d.level, []).append(d)
    out = []
    for lvl in sorted(by_level):
        if lvl == 0:
            continue
        cells = {}
        for d in by_level.get(lvl - 1, ()):                            # the pushers of the level before
            if not d.taken:
                continue
            add = int(fx((d.r / d.deg) * 2147483648.0))
            for j in range(int(indptr[d.node]), int(indptr[d.node + 1])):
                c = int(cell_of[indices[j]])
                cells[c] = cells.get(c, 0) + add
        back = [r for (l, _, r) in walk.returns if l == lvl - 1]       # dangling returns: one add of their sum to the seed's cell
        if back:
            c = int(cell_of[int(seed)])
            cells[c] = cells.get(c, 0) + int(fx(math.fsum(back) * 2147483648.0))
        for d in by_level[lvl]:
            cell = np.float32(cells.get(int(cell_of[d.node]), 0) & 0xFFFFFFFF)
            cand = bool(cell >= np.float32(int(dq_all[d.node])) * thr)
            out.append((lvl, d.node, d.taken, cand))
    return out


# ------------------------------------------------------------------ graph building

class _Builder:
    def __init__(self):
        self.rows = []

    def node(self, row=None):
        self.rows.append(list(row) if row is not None else [])
        return len(self.rows) - 1

    def sinks(self, k):
        """k new nodes whose only edge is a self-loop: a residue that reaches one stays there, exactly."""
        out = []
        for _ in range(k):
            v = self.node()
            self.rows[v] = [v]
            out.append(v)
        return out

    def csr(self, pad_to=0):
        rows = self.rows + [[] for _ in range(max(0, pad_to - len(self.rows)))]
        indptr = np.zeros(len(rows) + 1, np.int32)
        np.cumsum([len(r) for r in rows], out=indptr[1:])
        indices = np.array([c for r in rows for c in sorted(r)], np.int32)
        return indptr, indices


def dyadic_coef(n_coef):
    """1/2, 1/4, ..., with the last one repeated: powers of two that sum to 1, so coef * r is exact."""
    c = [2.0 ** -(i + 1) for i in range(n_coef)]
    c[-1] = c[-2] if n_coef > 1 else 1.0
    return np.array(c)


PAD_NODES = 65536                     # the general kernel takes the self-addressed CSR from this many nodes on (gfpush_plan.hpp)


class Case:
    """name, indptr / indices, seeds, coef, rmax; targets: per seed the node held at the threshold, (seed, node, level,
    n_in, relation, pushes) with relation in "eq" / "above" / "below" / "plus1" / "between"; path: what the GPU file runs."""

    def __init__(self, name, builder, seeds, rmax, n_coef, targets, path, note, degree_bits=(31,), coef=None):
        self.name, self.rmax, self.path, self.note = name, float(rmax), path, note
        self._builder = builder
        self.indptr, self.indices = builder.csr()
        self.seeds = np.array(seeds, np.int32)
        self.coef = dyadic_coef(n_coef) if coef is None else np.asarray(coef, np.float64)
        self.targets = targets
        self.degree_bits = degree_bits
        self.n_nodes = len(self.indptr) - 1

    def padded(self):
        """The same graph followed by isolated nodes up to PAD_NODES: no row changes, the general kernel's choice of CSR does."""
        return self._builder.csr(PAD_NODES)

    def neighbours(self, node):
        return self.indices[self.indptr[node]:self.indptr[node + 1]].tolist()

    def full_k(self):
        """A K above every row's support: every reserve value is compared, no tie rule is invoked."""
        walks, _, _ = walk_case(self)
        return max(len(w.reserve) for w in walks) + 3

    def full_groups(self, limit=1024):
        """{K: positions of seeds} for the general kernel (K <= 1024): one call under a K above every row's support where that
        fits, so that every reserve value is compared; cut_groups(limit) otherwise."""
        k = self.full_k()
        return {k: list(range(len(self.seeds)))} if k <= limit else self.cut_groups(limit)

    def cut_groups(self, limit=128):
        """{K: positions of seeds} for the sketch kernel, whose domain ends at K = 128: every seed under the largest K <= limit
        at which its K-th and (K+1)-th reserve values differ (or that holds its whole support), so that the index set is
        decided by values alone and no tie rule is invoked.  Seeds that share a K share a call."""
        walks, _, _ = walk_case(self)
        groups = {}
        for i, w in enumerate(walks):
            v = sorted((x for x in w.reserve.values() if x > 0.0), reverse=True)
            k = limit if len(v) <= limit else next(k for k in range(limit, 0, -1) if v[k - 1] > v[k] * (1 + 1e-9))
            groups.setdefault(k, []).append(i)
        return groups


Target = namedtuple("Target", "seed node level n_in relation pushes")


def _chain(b, degs, extra=0, twice=False):
    """seed -> n1 -> ... -> target, node i of the chain with degs[i] edges (the next node + sinks), the target with
    degs[-1] + extra sinks.  twice: the seed's row lists n1 two times (a repeated column: two contributions of one share)."""
    seed = cur = b.node()
    for i, d in enumerate(degs[:-1]):
        nxt = b.node()
        heads = [nxt, nxt] if twice and i == 0 else [nxt]
        b.rows[cur] = heads + b.sinks(d - len(heads))
        cur = nxt
    b.rows[cur] = b.sinks(degs[-1] + extra)
    return seed, cur


def _chain_case(name, rmax, variants, n_after, path, note):
    """variants: (degs, extra, twice, relation) -- one seed each, all in one graph.  n_after: levels after the target's."""
    b = _Builder()
    seeds, targets = [], []
    depth = len(variants[0][0]) - 1
    for degs, extra, twice, rel in variants:
        assert len(degs) - 1 == depth
        s, t = _chain(b, degs, extra, twice)
        seeds.append(s)
        targets.append(Target(s, t, depth, 2 if twice else 1, rel, rel in ("eq", "above")))
    return Case(name, b, seeds, rmax, depth + 1 + n_after, targets, path, note)


R12K, R4800 = 1.0 / 12000.0, 1.0 / 4800.0


def _level1_cases():
    return [
        _chain_case("l1_1e-4", 1e-4, [((100, 100), 0, False, "eq"), ((100, 100), 1, False, "plus1")], 2, "level1",
                    "100 x 100 = 1/1e-4 bit for bit, the twin with one edge more"),
        # (strictly increasing rows are a property of the whole graph: a repeated column anywhere switches the seed-row shortcut off)
        _chain_case("l1_dup", 1e-4, [((200, 100), 0, True, "eq"), ((200, 100), 1, True, "plus1")], 2, "level1",
                    "the seed row lists the target twice: 2 x 1/200 against rmax * 100, level 1 must not come from the seed row"),
        _chain_case("l1_1e-5", 1e-5, [((250, 400), 0, False, "eq"), ((250, 400), 1, False, "plus1")], 2, "level1",
                    "250 x 400 = 1/1e-5"),
        _chain_case("l1_1e-6", 1e-6, [((1000, 1000), 0, False, "eq"), ((1000, 1000), 1, False, "plus1")], 2, "level1",
                    "1000 x 1000 = 1/1e-6, the only tie of depth 1 at this rmax"),
        _chain_case("l1_ulp", R12K, [((80, 150), 0, False, "above"), ((100, 120), 0, False, "eq")], 2, "level1",
                    "rmax = 1/12000: 80 x 150 lands one ulp above the product, 100 x 120 on it"),
        _chain_case("l1_below", R4800, [((48, 100), 0, False, "below"), ((64, 75), 0, False, "eq")], 2, "level1",
                    "rmax = 1/4800: 48 x 100 lands one ulp BELOW the product and must not push; 64 x 75 on it"),
    ]


def _deeper_cases():
    return [
        _chain_case("l2_1e-4", 1e-4, [((20, 20, 25), 0, False, "eq"), ((20, 20, 25), 1, False, "plus1")], 2, "deep",
                    "level 2, 20 x 20 x 25"),
        _chain_case("l2_ulp", 1e-6, [((100, 100, 100), 0, False, "above"), ((80, 100, 125), 0, False, "eq")], 2, "deep",
                    "level 2 at 1e-6: 100^3 one ulp above, 80 x 100 x 125 on the product"),
        _chain_case("l2_below", R4800, [((15, 20, 16), 0, False, "below"), ((15, 16, 20), 0, False, "eq")], 2, "deep",
                    "level 2 at 1/4800: 15 x 20 x 16 one ulp below"),
        _chain_case("l3_1e-4", 1e-4, [((10, 10, 10, 10), 0, False, "eq"), ((10, 10, 10, 10), 1, False, "plus1")], 2, "deep",
                    "level 3, 10^4"),
        _chain_case("l3_ulp", R12K, [((10, 10, 12, 10), 0, False, "above"), ((10, 10, 10, 12), 0, False, "eq"),
                                     ((10, 10, 10, 12), 1, False, "plus1")], 2, "deep",
                    "level 3 at 1/12000: 10 x 10 x 12 x 10 one ulp above"),
        _chain_case("last_level", 1e-5, [((40, 50, 50), 0, False, "eq"), ((40, 50, 50), 1, False, "plus1")], 1, "deep",
                    "the target sits on the LAST pushing level: its edges are only recorded"),
        _chain_case("l2_wide", 1e-6, [((10, 20, 5000), 0, False, "eq"), ((10, 20, 5000), 1, False, "plus1")], 1, "wide",
                    "level 2 with 5 000 edges from one pusher: partitioned under a small lds_bytes, the HBM table under force_global"),
    ]


def _filter_cases():
    return [_chain_case("filter_margin", 1e-4, [((25, 400), 0, False, "eq"), ((25, 400), 1, False, "plus1"),
                                                ((50, 200), 0, False, "eq")], 2, "filter",
                        "25 / 400 and 50 / 200 at 1e-4: pushers that a threshold without the 2^-10 margin, rounded up, drops"),
            _chain_case("filter_margin_1e-3", 1e-3, [((25, 40), 0, False, "eq"), ((25, 40), 1, False, "plus1"),
                                                     ((50, 20), 0, False, "eq")], 2, "filter",
                        "25 / 40 and 50 / 20 at 1e-3, where rounding rmax * 2^31 to NEAREST rounds up: dropped without the margin")]


def _many_sum_case():
    """64 in-edges of 2^-12 each: 2^-6 = 2^-13 * 128, exact in any order and any grouping."""
    b = _Builder()
    seeds, targets = [], []
    for extra in (0, 1):
        seed = b.node()
        shared = b.sinks(63)
        u = b.node()
        mids = [b.node() for _ in range(64)]
        for m in mids:
            b.rows[m] = [u] + shared
        b.rows[seed] = mids
        b.rows[u] = b.sinks(128 + extra)
        seeds.append(seed)
        targets.append(Target(seed, u, 2, 64, "plus1" if extra else "eq", not extra))
    return Case("many_sum", b, seeds, 2.0 ** -13, 4, targets, "deep",
                "64 dyadic contributions whose sum is rmax * deg exactly (rmax = 2^-13, deg 128); the twin has 129 edges")


def _many_floor_case():
    """64 equal, NON-dyadic contributions s = ((1/3)/81)/48.  rmax is set from their sum: sum = rmax * 96 * (1 + 2^-30), far
    enough above the threshold that the order and grouping of the adds cannot matter (2^-52), far inside the filter's margin
    (2^-10) and inside what flooring 64 shares loses (about 2^-19 of the cell)."""
    b = _Builder()
    seed = b.node()
    hub = b.node()
    b.rows[seed] = [hub] + b.sinks(2)
    shared = b.sinks(47)
    u = b.node()
    mids = [b.node() for _ in range(64)]
    for m in mids:
        b.rows[m] = [u] + shared
    b.rows[hub] = mids + b.sinks(17)
    b.rows[u] = b.sinks(96)
    s = ((1.0 / 3) / 81) / 48
    total = 0.0
    for _ in range(64):
        total += s
    rmax = total / 96 * (1.0 - 2.0 ** -30)
    return Case("many_floor", b, [seed], rmax, 5, [Target(seed, u, 3, 64, "above", True)], "filter",
                "64 non-dyadic contributions 2^-30 above the threshold: the per-edge ceil keeps the node a candidate")


def _seed_case():
    b = _Builder()
    s0 = b.node(); b.rows[s0] = b.sinks(1000)
    s1 = b.node(); b.rows[s1] = b.sinks(1001)
    return Case("seed_test", b, [s0, s1], 1e-3, 3, [Target(s0, s0, 0, 1, "eq", True), Target(s1, s1, 0, 1, "plus1", False)], "seed",
                "the seed's own test: 1.0 == 1e-3 * 1000 pushes; with 1 001 edges nothing is pushed and only the seed's slot is filled")


def _dangling_case():
    """seed (2 edges) -> a (60) -> u (40 edges, one of them to the dangling z) and p (39 edges, one to w; w -> seed).
    rmax = 1/4800: u sits ON its threshold (0.5/60 == rmax * 40) and pushes, but its share (0.5/60)/40 rounds one ulp BELOW
    rmax -- the only way a dangling node with one contribution can hold less than rmax.  z returns it to the seed, where it
    meets w's (0.5/60)/39: together >= rmax * 2, w's alone is not."""
    b = _Builder()
    seed, a, u, p, z, w = (b.node() for _ in range(6))
    b.rows[seed] = [a] + b.sinks(1)
    b.rows[a] = [u, p] + b.sinks(58)
    b.rows[u] = [z] + b.sinks(39)
    b.rows[p] = [w] + b.sinks(38)
    b.rows[w] = [seed]
    case = Case("dangling", b, [seed], R4800, 7, [Target(seed, u, 2, 1, "eq", True), Target(seed, seed, 4, 2, "above", True)], "deep",
                "a dangling node at level 3 holding one ulp less than rmax; its return lifts the seed across rmax * 2 at level 4")
    case.dangling_node, case.w_node = z, w
    return case


def _carry_case():
    """seed -> {q, b}, b -> q; q has 100 edges and rmax = 1e-2: q holds 0.5 at level 1 and 0.5 at level 2, each below
    rmax * 100 == 1.0.  Dropped both times; a residue carried over would push at level 2."""
    b = _Builder()
    seed, q, mid = (b.node() for _ in range(3))
    b.rows[seed] = [q, mid]
    b.rows[mid] = [q]
    b.rows[q] = b.sinks(100)
    return Case("carry", b, [seed], 1e-2, 5, [Target(seed, q, 1, 1, "below_far", False)], "deep",
                "a residue that fails the test is dropped, not carried: 0.5 + 0.5 would reach rmax * deg")


SAT_N = 16800                          # rmax = 1/16800: divisible by every target degree below and by their chains


def _saturation_case():
    """Packed degree fields of 2 and 3 bits (deg_sat 3 and 7).  Per deg_sat: targets of degree deg_sat - 1, deg_sat,
    deg_sat + 1 and 4 * deg_sat holding exactly rmax * deg ("eq"), and targets of degree deg_sat + 1 and 4 * deg_sat holding
    exactly rmax * deg_sat ("between": the cheap half of the test passes on equality, the exact half must fail).  Twelve
    seeds; level 2, so the decision is taken by a table drain."""
    b = _Builder()
    seeds, targets = [], []
    for sat in (3, 7):
        for deg, hold in ((sat - 1, sat - 1), (sat, sat), (sat + 1, sat + 1), (4 * sat, 4 * sat), (sat + 1, sat), (4 * sat, sat)):
            d0, d1 = SAT_CHAINS[hold]
            s, t = _chain(b, (d0, d1, deg))
            seeds.append(s)
            targets.append(Target(s, t, 2, 1, "eq" if hold == deg else "between", hold == deg))
    return Case("saturation", b, seeds, 1.0 / SAT_N, 4, targets, "saturation",
                "degree-field saturation: residues at rmax * deg and at rmax * deg_sat for degrees around deg_sat 3 and 7",
                degree_bits=(2, 3))


# hold -> (d0, d1) with (1/d0)/d1 == (1/16800) * hold bit for bit (searched over the divisor pairs of 16800 / hold; the host test
# asserts the equality)
SAT_CHAINS = {2: (42, 200), 3: (28, 200), 4: (21, 200), 6: (14, 200), 7: (12, 200), 8: (12, 175), 12: (7, 200), 28: (3, 200)}


@functools.lru_cache(maxsize=1)
def cases():
    out = _level1_cases() + _deeper_cases() + _filter_cases() + [_many_sum_case(), _many_floor_case(), _seed_case(),
                                               _dangling_case(), _carry_case(), _saturation_case()]
    return {c.name: c for c in out}


# the list the GPU file parametrises over and the host file audits
GPU_CASES = ("l1_1e-4", "l1_dup", "l1_1e-5", "l1_1e-6", "l1_ulp", "l1_below", "l2_1e-4", "l2_ulp", "l2_below", "l3_1e-4", "l3_ulp",
             "last_level", "l2_wide", "filter_margin", "filter_margin_1e-3", "many_sum", "many_floor", "seed_test", "dangling", "carry", "saturation")
