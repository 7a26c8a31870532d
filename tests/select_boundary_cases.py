"""GFPush's top-K select (graph.h:111-126) held at the K-th place: case graphs, a strict reference, a mirror of the rule.

All plain Python / numpy on the CPU:

  * select_exact: the slot-ordered row the header promises -- the positive totals of push_boundary_cases.push_walk64's reserve
    map sorted by (value desc, column asc), first K.  The GPU file compares slot for slot and bit for bit with it.
  * records / edge_terms: what each node's total is a sum of, per level (the general kernel's log: coef[l] * r) and per edge
    (the sketch kernel's log: coef[l] * share).  A case is EXACT when every such sum is order-independent: one term, two
    terms, or dyadic terms within one 53-bit window.  Only then can a kernel that adds with LDS atomics in arrival order be
    compared bit for bit.  tests/test_host_select_boundary.py asserts it for every case.
  * select_mirror: a Python model of the RULE of both selects (not of their launches): the composite order, the general
    kernel's tau off the 64 x 16 counters with its claim threshold and candidate floor, the sketch kernel's rounds over
    fixed-point cells with its completeness test, id digits and partition merge.  SELECT_MUTANTS are deliberate mistakes.
  * cases(): graphs built constructively.  Every case is a "fan": seed -> hubs -> leaves, each leaf owning one record, so a
    hub of any degree G makes a flat group of G bit-equal totals; near ties add one ulp-sized dyadic record through an
    un-normalised coefficient.  Graphs are padded with isolated nodes (2^17, one 2^21) so that ids are large and the general
    kernel can take either CSR.
"""
from __future__ import annotations

import functools
import math
from fractions import Fraction

import numpy as np

import collision_cases as cc
from push_boundary_cases import PAD_NODES, _Builder, dyadic_coef, push_walk64, ulps  # noqa: F401  (re-exported for the tests)

kBucketCap = kSkTie = 256             # gfpush_kernels.hpp / gfpush_sketch.hpp: entries ranked by comparison
kSkNarrow = 16                        # gfpush_sketch.hpp: the K-th bucket is narrowed while it holds more
N_PAD = 1 << 17                       # >= PAD_NODES: the general kernel may take the self-addressed CSR
RMAX = 2.0 ** -20                     # every node of every case that holds a residue before the last level pushes

SELECT_MUTANTS = ("col_desc", "low4_dropped", "low12_dropped", "value_f32", "zero_written", "thr_not_per_level", "thr_margin_up",
                  "floor_margin_up", "tau_upper_edge", "tau_at_k_minus_1", "complete_no_margin", "complete_ceil", "short_row_kept",
                  "id_digit_from_low_byte", "merge_drops_running_list", "bit4_in_low_digit")
# Mistakes no constructible exact case can show, with the reason (at most two, the second paired with the first).
INDISTINGUISHABLE = {
    "complete_no_margin": "a cell is a sum of CEILed fixed-point shares, so an unswept node has total * scale <= cell <= t_c - 1; "
                          "tau * scale >= t_c then already puts it strictly below tau in exact arithmetic -- the 2^-20 margin guards "
                          "only the rounding of the product tau * scale, which no case whose totals are exact dyadic values moves",
    "complete_ceil": "paired with complete_no_margin: ceil(tau * scale) >= t_c gives tau * scale > t_c - 1 >= every unswept "
                     "total * scale, the same strict bound",
}
SKETCH_MUTANTS = ("complete_no_margin", "complete_ceil", "short_row_kept", "id_digit_from_low_byte", "merge_drops_running_list")
SK_SCALE = 2147483648.0               # fixed-point cells: shares * 2^31, rounded up


def _bits(v):
    return int(np.float64(v).view(np.int64))


# ------------------------------------------------------------------ reference

def select_exact(reserve, K):
    """[(column, value)] in slot order: positive totals by (value desc, column asc), first K."""
    rows = sorted(((c, v) for c, v in reserve.items() if v > 0.0), key=lambda cv: (-cv[1], cv[0]))
    return rows[:K]


def next_after_k(reserve, K):
    """The (K+1)-th positive total, 0.0 when there is none."""
    rows = sorted((v for v in reserve.values() if v > 0.0), reverse=True)
    return rows[K] if len(rows) > K else 0.0


def records(case, seed):
    """(per_level, per_edge): {node: [(level, coef[level] * r)]} and {node: [(level, coef[level] * share)]} of one row.
    r is the node's residue at the level (summed in the walk's order), share one edge's contribution to it."""
    indptr, indices, coef, rmax = case.indptr, case.indices, case.coef, case.rmax
    n_coef = len(coef)
    res = {int(seed): [1.0]}
    per_level, per_edge = {}, {}
    for lvl in range(n_coef):
        c = float(coef[lvl])
        nxt = {}
        back = []
        for u, shares in res.items():
            r = 0.0
            for s in shares:
                r += s
            per_level.setdefault(u, []).append((lvl, c * r))
            per_edge.setdefault(u, []).extend((lvl, c * s) for s in shares)
            if lvl == n_coef - 1:
                continue
            lo, hi = int(indptr[u]), int(indptr[u + 1])
            deg = hi - lo
            if deg == 0:
                back.append(r)
            elif r >= rmax * deg:
                for j in range(lo, hi):
                    nxt.setdefault(int(indices[j]), []).append(r / deg)
        if back:
            nxt.setdefault(int(seed), []).append(math.fsum(back))
        res = nxt
    return per_level, per_edge


def sums_in_three_orders(terms, rng):
    """The sum of `terms` ascending, descending and in a seeded shuffle."""
    out = []
    for order in (sorted(terms), sorted(terms, reverse=True), [terms[i] for i in rng.permutation(len(terms))]):
        acc = 0.0
        for t in order:
            acc += t
        out.append(acc)
    return out


def one_window(terms):
    """Every subset sum of `terms` is a double: all are multiples of q = the lowest set bit of any term, and the sum of their
    magnitudes is below 2^53 q."""
    nz = [Fraction(abs(t)) for t in terms if t != 0.0]
    if len(nz) <= 1:
        return True
    q = min(Fraction(1, f.denominator) if f.denominator > 1 else Fraction(f.numerator & -f.numerator) for f in nz)
    return sum(nz) / q < (1 << 53)


# ------------------------------------------------------------------ the mirror

def _counter_edge(v, upper=False):
    """Lower (upper) edge of the 1/16-binade counter that holds v: 0.0 outside [2^-62, 2) (the last binade gives no threshold)."""
    b = _bits(v)
    e = 1023 - (b >> 52)
    if e < 0 or e >= 63:
        return 0.0
    m4 = (b >> 48) & 15
    lo = np.int64(((1023 - e) << 52) | (m4 << 48)).view(np.float64)
    return float(lo) * (17 + m4) / (16 + m4) if upper else float(lo)


def _order_key(mut, unit_of=None):
    def key(cv):
        c, v = cv
        b = _bits(v)
        if mut == "low4_dropped":
            b &= ~0xF
        elif mut == "low12_dropped":
            b &= ~0xFFF
        elif mut == "value_f32":
            b = _bits(float(np.float32(v)))
        elif mut == "bit4_in_low_digit":                              # digit 5 taken as (bits & 0x1F): bit 4 counted twice, bit 0 lost
            b = (b & ~0xF) | ((b >> 1) & 0xF)
        if mut == "col_desc":
            return (-b, -c)
        if mut == "id_digit_from_low_byte":                           # id bytes walked from the low one up
            u = c if unit_of is None else unit_of(c)
            return (-b, (u & 255, (u >> 8) & 255, (u >> 16) & 255, u >> 24))
        return (-b, c)
    return key


def _positive(v, mut):
    return v >= 0.0 if mut == "zero_written" else v > 0.0


def select_mirror(per_level, K, n_levels, mut=None, model="general", sk_target=None, parts=1, unit_of=None, coef_nonneg=True):
    """The slot-ordered row by the kernels' RULE.  per_level: {node: [(level, record)]} (records()[0]).

    model "general": tau = the lower edge of the 64 x 16 counter holding the K-th largest record of the first level with
    >= 2K records (all coef >= 0), nodes owning a record >= tau / n_levels * 0.99999 are claimed, totals > 0 and
    >= tau * 0.99999 become candidates, the K best by (value bits desc, column asc) are written.
    model "sketch": cells = totals in 2^31 fixed point rounded up; t_c = the lower counter edge of the sk_target-th largest
    cell; rounds of (sweep cells >= t_c, select K) until floor(tau * scale * (1 - 2^-20)) >= t_c, as phase_sk_topk; with
    parts > 1 every round selects per partition (node % parts) and merges with the running list."""
    assert mut is None or mut in SELECT_MUTANTS, mut
    assert (mut in SKETCH_MUTANTS) <= (model == "sketch"), (mut, model)
    total = {}
    for node, recs in per_level.items():
        acc = 0.0
        for _, v in recs:
            acc += v
        total[node] = acc
    key = _order_key(mut, unit_of)
    if model == "general":
        tau = 0.0
        by_level = {}
        for node, recs in per_level.items():
            for lvl, v in recs:
                by_level.setdefault(lvl, []).append(v)
        seg = next((sorted(by_level[l], reverse=True) for l in sorted(by_level) if len(by_level[l]) >= 2 * K), None)
        if coef_nonneg and seg is not None:
            pos = [v for v in seg if v > 0.0]
            kth = K - 1 if mut == "tau_at_k_minus_1" else K
            if len(pos) >= kth >= 1:
                tau = _counter_edge(pos[kth - 1], upper=mut == "tau_upper_edge")
        nodes = total
        floor_v = 0.0
        if tau > 0.0:
            thr = (tau if mut == "thr_not_per_level" else tau / n_levels) * (1.00001 if mut == "thr_margin_up" else 0.99999)
            nodes = {n: total[n] for n, recs in per_level.items() if any(v >= thr for _, v in recs)}
            floor_v = tau * (1.00001 if mut == "floor_margin_up" else 0.99999)
        cand = [(n, v) for n, v in nodes.items() if _positive(v, mut) and v >= floor_v]
        return sorted(cand, key=key)[:K]
    # sketch
    cell = {n: int(math.ceil(v * SK_SCALE)) for n, v in total.items() if v > 0.0}
    ranked = sorted(cell.values(), reverse=True)
    t_c = 1
    if sk_target is not None and len(ranked) >= sk_target:
        t_c = max(1, int(_counter_edge(float(ranked[sk_target - 1]) * 2.0 ** -40) * 2.0 ** 40))    # (cells < 2^32 scaled into the counters' range)
    last = False
    rnd = 0
    while True:
        swept = [(n, total[n]) for n in cell if cell[n] >= t_c]
        if mut == "zero_written":
            swept += [(n, v) for n, v in total.items() if v == 0.0]
        run = []
        for part in range(parts):
            mine = sorted([cv for cv in swept if cv[0] % parts == part], key=key)[:K]
            run = mine if mut == "merge_drops_running_list" else sorted(run + mine, key=key)[:K]
        if t_c <= 1 or last or mut == "short_row_kept":
            return run
        if len(run) == K:
            x = run[-1][1] * SK_SCALE * (1.0 if mut == "complete_no_margin" else 1.0 - 2.0 ** -20)
            tau_fx = math.ceil(x) if mut == "complete_ceil" else math.floor(x)
            if tau_fx >= t_c:
                return run
            t_c, last = max(1, int(tau_fx)), True
        else:
            t_c = 1 if rnd >= 2 else max(1, t_c >> 4)
        rnd += 1


# ------------------------------------------------------------------ graph building

class _Placed(_Builder):
    """Rows at chosen ids of a graph of n nodes; every other id is an isolated node."""

    def __init__(self, n):
        super().__init__()
        self.n, self.at = n, {}

    def put(self, v, row):
        assert 0 <= v < self.n and v not in self.at and all(0 <= c < self.n for c in row), v
        self.at[int(v)] = [int(c) for c in row]

    def csr(self, pad_to=0):
        n = max(self.n, pad_to)
        deg = np.zeros(n, np.int64)
        for v, r in self.at.items():
            deg[v] = len(r)
        indptr = np.zeros(n + 1, np.int32)
        np.cumsum(deg, out=indptr[1:])
        indices = np.array([c for v in sorted(self.at) for c in sorted(self.at[v])], np.int32)
        return indptr, indices


class Case:
    """name; indptr / indices; seeds; coef; rmax; ks: the K values run; path: what the case is for; kernels: which kernels can
    take it; claims: what the host test holds it to (see test_case_holds_what_it_claims)."""

    def __init__(self, name, builder, seeds, coef, ks, path, note, kernels=(1, 2), **claims):
        self.name, self.path, self.note, self.kernels, self.claims = name, path, note, kernels, claims
        self.indptr, self.indices = builder.csr()
        self.seeds = np.array(seeds, np.int32)
        self.coef = np.asarray(coef, np.float64)
        self.rmax = RMAX
        self.ks = tuple(ks)
        self.n_nodes = len(self.indptr) - 1

    @functools.lru_cache(maxsize=None)
    def walks(self):
        return [push_walk64(self.indptr, self.indices, s, self.coef, self.rmax) for s in self.seeds]

    def expected(self, K):
        """Per seed the strict row."""
        return [select_exact(w.reserve, K) for w in self.walks()]

    def compact(self, limit=3900):
        """(indptr, indices, seeds, ids) of the same graph without its isolated padding: node i of it is ids[i], order kept, so
        every row keeps its slot order.  None when more than `limit` nodes are in use (the direct-indexed tables hold a graph of
        up to about 3 980 nodes)."""
        deg = np.diff(self.indptr)
        used = np.zeros(self.n_nodes, bool)
        used[deg > 0] = True
        used[self.indices] = True
        used[self.seeds] = True
        ids = np.flatnonzero(used)
        if len(ids) > limit:
            return None
        new = np.full(self.n_nodes, -1, np.int64)
        new[ids] = np.arange(len(ids))
        indptr = np.zeros(len(ids) + 1, np.int32)
        np.cumsum(deg[ids], out=indptr[1:])
        return indptr, new[self.indices].astype(np.int32), new[self.seeds].astype(np.int32), ids

    def units(self):
        """node -> unit number of the self-addressed CSR (what both kernels rank by there)."""
        return cc.acsr_layout(self.indptr)[0]


def _fan(b, seed, hubs):
    """seed -> hubs -> leaves: hubs = [(hub id, [leaf ids])]; leaves stay isolated (the last level only records them)."""
    b.put(seed, [h for h, _ in hubs])
    for h, leaves in hubs:
        b.put(h, leaves)


# ---- tie groups straddling the K-th place

LAYOUTS = {                            # member ids of the group: (count, step, base when the group is LOW, base when it is HIGH)
    "consec": (300, 1, 1000, 40000),
    "step256": (300, 256, 1000, 40000),
    "step64k": (17, 65536, 1000, 300000),
    "straddle4096": (300, 1, 3 * 4096 - 40, 20 * 4096 - 40),
}


def _tie_case(name, G, ids, others_base, n, note, below=True):
    """Four hubs (two without `below`): A with 8 leaves (above the group), T with the G members, and with `below` B with G + 3
    leaves (under the group) and C with 3.  coef = 1/2, 1/4, 1/4: totals 1/2 (seed), 1/4 / d0 (hubs), 1/4 / (d0 * g) (leaves)."""
    b = _Placed(n)
    nxt = iter(range(others_base, others_base + 2 * G + 64))
    seed = next(nxt)
    hub_ids = [next(nxt) for _ in range(4 if below else 2)]
    groups = [[next(nxt) for _ in range(8)], list(ids)]
    if below:
        groups += [[next(nxt) for _ in range(G + 3)], [next(nxt) for _ in range(3)]]
    _fan(b, seed, list(zip(hub_ids, groups)))
    d0 = len(hub_ids)
    v = 0.25 * ((1.0 / d0) / G)
    above = 1 + d0 + sum(len(g) for g in groups if len(g) < G)
    K = above + max(1, min(G // 2, 53))
    return Case(name, b, [seed], dyadic_coef(3), [K], "tie", note, group=list(ids), group_value=v, above=above)


def _tie_cases():
    out = []
    for G in (2, 16, 17, 256, 257, 5000):
        what = {2: "the smallest group", 16: "kSkNarrow", 17: "kSkNarrow + 1", 256: "kBucketCap = kSkTie", 257: "kBucketCap + 1",
                5000: "resolved by id digits alone; partitioned under a small table"}[G]
        out.append(_tie_case(f"tie_g{G}", G, range(1000, 1000 + G), 70000, N_PAD, f"{G} equal totals across the K-th place: {what}",
                             below=G <= 300))
    for lay, (cnt, step, lo, hi) in LAYOUTS.items():
        n = 1 << 21 if lay == "step64k" else N_PAD
        out.append(_tie_case(f"tie_{lay}_low", cnt, range(lo, lo + cnt * step, step), n - 4096, n,
                             f"{cnt} equal totals, ids {step} apart from {lo}: the group's ids BELOW every other selected column"))
        out.append(_tie_case(f"tie_{lay}_high", cnt, range(hi, hi + cnt * step, step), 16, n,
                             f"{cnt} equal totals, ids {step} apart from {hi}: the group's ids ABOVE every other selected column"))
    return out


# ---- near ties

def _near_case(j):
    """Per seed: seed -> {a, b}; a -> 96 X, 200 Y, 3 helpers (32 X each), 213 fillers; X, Y, b loop on themselves; fillers -> q.
    coef = 1/2, 1/4, 1/8, 2^(j - 50).  With s = 2^-10 (a's share): Y = s (1/8 + c3), X = Y + c3 s / 32 = Y + 2^j ulps.
    K = 3 + 96: the K-th total is the last X, the (K+1)-th the first Y.  Seed 0: every X id above every Y id (the larger value
    carries the larger column); seed 1: mirrored (the control)."""
    b = _Placed(N_PAD)
    seeds = []
    c3 = 2.0 ** (j - 50)
    for which, base in enumerate((2000, 9000)):
        seed, a, bb, q = base, base + 1, base + 2, base + 3
        lowblock = list(range(base + 100, base + 300))
        highblock = list(range(base + 1000, base + 1200))
        xs, ys = (highblock[:96], lowblock) if which == 0 else (lowblock[:96], highblock)
        helpers = [base + 10 + i for i in range(3)]
        fillers = [base + 2000 + i for i in range(213)]
        b.put(seed, [a, bb])
        b.put(a, xs + ys + helpers + fillers)
        b.put(bb, [bb])
        for x in xs + ys:
            b.put(x, [x])
        for i, h in enumerate(helpers):
            b.put(h, xs[32 * i:32 * i + 32])
        for f in fillers:
            b.put(f, [q])
        seeds.append(seed)
    return Case(f"near_bit{j}", b, seeds, [0.5, 0.25, 0.125, c3], [99], "near",
                f"ranks K and K + 1 differ by 2^{j} ulps inside a crowd of more than 256 totals that agree above bit 16; seed 1 mirrors the columns",
                near_ulps=1 << j)


# ---- K against the support

def _support_cases():
    out = []
    b = _Placed(N_PAD)
    _fan(b, 500, [(600, [700]), (601, [601])])
    out.append(Case("support_zero", b, [500], [0.5, 0.25, 0.0], [2, 3, 4, 8], "support",
                    "a zero coefficient at the only level that reaches node 700: its total is exactly 0.0 and is not written; "
                    "K = positives - 1, positives, + 1 and beyond", positives=3, zeros=[700]))
    b = _Placed(N_PAD)
    _fan(b, 500, [(600, [600]), (601, [700])])
    out.append(Case("support_negative", b, [500], [0.5, 0.25, -0.25], [1, 2, 3, 8], "support",
                    "one negative coefficient: 600 cancels to exactly 0.0 (1/8 - 1/8), 700 is negative; neither is written",
                    kernels=(1,), positives=2, zeros=[600], negatives=[700]))
    b = _Placed(N_PAD)
    _fan(b, 900, [(800, [1000, 1001]), (801, [1002, 1003])])
    out.append(Case("support_first_tie", b, [900], [0.125, 0.25, 0.25], [1, 2, 3, 6, 7, 8], "support",
                    "K = 1 with a three-way tie for first place (seed 900 and hubs 800, 801 at 1/8): the smallest column wins",
                    positives=7, first_tie=[800, 801, 900]))
    return out


# ---- binade and counter edges

def _edge_case(bexp, m):
    """seed -> 4 hubs, hub i -> 2 leaves.  coef[1] puts the hubs ON (16 + m) / 16 * 2^-bexp, coef[2] puts the leaves one ulp
    below it.  K = 5: the K-th total is the last hub, the (K+1)-th the first leaf."""
    b = _Placed(N_PAD)
    hubs = [(3000 + i, [3100 + 2 * i, 3101 + 2 * i]) for i in range(4)]
    _fan(b, 2900, hubs)
    edge = (16 + m) / 16.0 * 2.0 ** -bexp
    below = float(np.nextafter(edge, 0.0))
    coef = [min(1.0, 2 * edge) if edge < 1.0 else 1.0, edge * 4, below * 8]
    return Case(f"edge_b{bexp}_m{m}", b, [2900], coef, [5], "edge",
                f"the K-th total is exactly {16 + m}/16 * 2^-{bexp}, the (K+1)-th one ulp below"
                + (": the row straddles two binades" if m == 0 else ": two 1/16-binade counters"), edge=edge)


# ---- the general kernel's pruned aggregation

T_PRUNE = 2.0 ** -12


def _prune_case():
    """seed 100 -> itself and F1..F15, coef = t, 16 t, 256 t: the seed's three records are t each, its total X = 3 t.
    Level 2 is the first level with >= 2K = 18 records.  Its records: 8 of 4 t (the leaves u of F1, F2, four each), then W's 3 t
    (one share of 1/256 from each of F3, F4, F5): the 9th largest, exactly on the counter edge 24/16 * 2 t, so tau = 3 t = X.
    thr = tau / 3 * 0.99999 sits just under X's records.  Y collects 2.75 / 256 (F6, F7: 16 edges, F8: 32, F9: 64): 2.75 t, under
    tau * 0.99999.  Z is a leaf of F10 (32 edges): one record t / 2, under thr: never claimed.  K = 9: the 8 u, then X (column 100
    before W's 400 at the same total)."""
    b = _Placed(N_PAD)
    seed, W, Y, Z = 100, 400, 401, 402
    F = list(range(200, 215))
    b.put(seed, [seed] + F)
    fresh = iter(range(1000, 3000))
    u = [next(fresh) for _ in range(8)]
    b.put(F[0], u[:4]); b.put(F[1], u[4:])
    for f in F[2:5]:
        b.put(f, [W] + [next(fresh) for _ in range(15)])
    for f, d in ((F[5], 16), (F[6], 16), (F[7], 32), (F[8], 64)):
        b.put(f, [Y] + [next(fresh) for _ in range(d - 1)])
    b.put(F[9], [Z] + [next(fresh) for _ in range(31)])
    for f in F[10:]:
        b.put(f, [next(fresh) for _ in range(16)])
    t = T_PRUNE
    return Case("prune_edge", b, [seed], [t, 16 * t, 256 * t], [9], "prune",
                "tau = 3 t on a counter edge; X = 3 t in three records of tau / 3 is selected, Y = 2.75 t and Z = t / 2 are not",
                X=seed, W=W, Y=Y, Z=Z, tau=3 * t)


# ---- the heavy list (phase_tau: the threshold level is not the last one)

def _heavy_route_case():
    """prune_edge with a fourth level: every level-2 node loops on itself and coef[3] = 64 t adds a quarter of its level-2
    record.  Level 2 still is the first level with >= 2K = 22 records, but no longer the last: tau is taken when it ends
    (phase_tau) and the keys of level 3's records >= tau / 4 * 0.99999 go to the heavy list.  tau = t, the 11th largest record of
    level 2 (8 of 4 t, W's 3 t, Y's 2.75 t, then t), a binade edge; the level-3 records of the nodes that held 1/256 are
    17/64 t (their own 1/256 and 1/4096 more from their parent's second push), above tau / 4 * 0.99999: noted as heavy, 165 keys.
    K = 11: the 8 u, W, Y, then X = 3 t + t / 64; the (K+1)-th is F1 = 2 t + t / 64."""
    base = _prune_case()
    b = _Placed(N_PAD)
    deg = np.diff(base.indptr)
    for v in np.flatnonzero(deg > 0):
        b.put(int(v), base.indices[base.indptr[v]:base.indptr[v + 1]].tolist())
    for v in sorted(set(base.indices.tolist())):
        if deg[v] == 0:
            b.put(int(v), [int(v)])
    t = T_PRUNE
    cl = base.claims
    return Case("heavy_route", b, base.seeds.tolist(), [t, 16 * t, 256 * t, 64 * t], [11], "heavy",
                "the threshold level (2) is not the last: tau from phase_tau, pass A reads the heavy list; X is the K-th, F1 the (K+1)-th",
                X=cl["X"], next=200, tau=t, thr_level=2)


def _heavy_flat_case(n_coef, name, note):
    """64 nodes, every row lists all 64: from level 1 on every node holds 1/64.  coef = 1/2, 1/4, 1/8, 1/8, ...: level 1 has
    64 >= 2K records of 2^-8 (tau = 2^-8, a binade edge), every later record 2^-9 reaches tau / n_coef * 0.99999 and is noted.
    NOT padded: the heavy list holds 4 * cand_cap keys with cand_cap = min(N, 1 + L * F_max, log records) + 1 = 65
    (gfpush_kernels.hpp heavy_view, gfpush_plan.hpp slab_sizes): 260 keys.  All 63 non-seed totals are equal; K = 16."""
    b = _Placed(64)
    for v in range(64):
        b.put(v, list(range(64)))
    coef = [0.5, 0.25] + [0.125] * (n_coef - 2)
    return Case(name, b, [5], coef, [16], "heavy", note, heavy_records=64 * (n_coef - 2), heavy_cap=260, tau=2.0 ** -8, thr_level=1)


@functools.lru_cache(maxsize=1)
def cases():
    out = _tie_cases() + [_near_case(j) for j in (0, 3, 4, 12)] + _support_cases() \
        + [_edge_case(1, 0), _edge_case(1, 5), _edge_case(7, 0), _edge_case(7, 5), _prune_case(), _heavy_route_case(),
           _heavy_flat_case(4, "heavy_flat", "128 heavy keys: the list holds them, pass A claims from it"),
           _heavy_flat_case(8, "heavy_flat_overflow", "384 heavy keys against a list of 260: it overflows and TOP-K takes its own tau")]
    return {c.name: c for c in out}


# the list the GPU file parametrises over and the host file audits
GPU_CASES = ("tie_g2", "tie_g16", "tie_g17", "tie_g256", "tie_g257", "tie_g5000",
             "tie_consec_low", "tie_consec_high", "tie_step256_low", "tie_step256_high", "tie_step64k_low", "tie_step64k_high",
             "tie_straddle4096_low", "tie_straddle4096_high",
             "near_bit0", "near_bit3", "near_bit4", "near_bit12",
             "support_zero", "support_negative", "support_first_tie",
             "edge_b1_m0", "edge_b1_m5", "edge_b7_m0", "edge_b7_m5", "prune_edge", "heavy_route", "heavy_flat", "heavy_flat_overflow")
