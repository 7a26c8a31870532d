"""Graphs whose keys provably pile into one bucket of GFPush's LDS hash tables, built on the CPU.

Two things decide where a key goes, and both are mirrored here in numpy:
  * the key layout -- the self-addressed CSR (acsr_units_kernel / acsr_fill_kernel in gfpush.hip: a row of deg entries owns
    max(1, ceil(deg / 32)) units, node_pos is the exclusive prefix sum of the units, key = node_pos | min(deg, a_sat) << pos_bits)
    and the packed CSR (pack_degree_kernel: key = node id | min(deg, deg_sat) << id_bits);
  * the hashes of grand_plus_amd/csrc/gfpush_hash.hpp (tests/test_host_collision_cases.py holds this mirror to the C++ header).

A probe sequence gives up after kMaxProbe = 24 slots, so 25 keys with one home slot overflow a table however empty it is.  A
collision set is SET_SIZE = 64 >= 2 * (kMaxProbe + 1) nodes whose 16-bit hash value lies below WINDOW = 65536 // (cap_max -
kProbeSpan): their home is slot 0 at EVERY capacity up to cap_max, and after one split by hash_b a half still overflows.

One base graph serves the three families (sketch kernel: sk_home of the self-addressed key; general kernel: hash_a of the
self-addressed key and of the packed key).  Every node has a self-loop and 0, 1 or 3 ring successors (degrees 1, 2, 4: powers of two); SPECIAL rows get their final
length first and their targets afterwards, so the layout -- and with it every key -- does not move when the targets are chosen:
  A    seed whose row IS the collision set (64 <= 256 edges: level 1 is a one-wave level, merged into the seed's call)
  B    seed -> one node m -> the set (the overflow happens at level 2)
  C    seed -> a hub of HUB_LEN = 512 > 256 edges: the set plus filler (not a one-wave level)
and a control for each: the same row lengths, targets with pairwise distinct homes at every capacity in play.
"""
from __future__ import annotations

import functools
import json
import os

import numpy as np

K_MAX_PROBE = 24
K_PROBE_SPAN = K_MAX_PROBE * (K_MAX_PROBE + 1) // 2
K_MIN_CAP = 1024
K_SK_SOLO_EDGES = 256

_M32 = np.uint64(0xFFFFFFFF)


def _u64(k):
    return np.asarray(k).astype(np.uint64) & _M32


def mul24(a, b):
    return ((_u64(a) & np.uint64(0xFFFFFF)) * (_u64(b) & np.uint64(0xFFFFFF))) & _M32


def hash_a(k):
    k = (_u64(k) * np.uint64(0x9E3779B1)) & _M32
    k = k ^ (k >> np.uint64(15))
    return (k * np.uint64(0x85EBCA77)) & _M32


def hash_b(k):
    k = (_u64(k) * np.uint64(0x7FEB352D)) & _M32
    k = k ^ (k >> np.uint64(16))
    return (k * np.uint64(0x846CA68B)) & _M32


def slot_of(h, cap):
    return (_u64(h) * np.uint64(cap)) >> np.uint64(32)


def home_lds(k, cap):
    return slot_of(hash_a(k), cap - K_PROBE_SPAN)


def sk_cell(k):
    return mul24(k, 0x9E3779)


def sk_hash16(k):
    h = mul24(k, 0x9E3779)
    h = h ^ (h >> np.uint64(15))
    return mul24(h, 0x85EBCB) >> np.uint64(16)


def sk_home(k, cap):
    prod = mul24(sk_hash16(k), cap - K_PROBE_SPAN)
    return (prod.astype(np.uint32).view(np.int32) >> 16).view(np.uint32).astype(np.uint64)      # (an arithmetic shift, as on the device)


def part_of(k, parts):
    return slot_of(hash_b(k), parts)


# ------------------------------------------------------------------ key layouts

def acsr_layout(indptr, max_degree_bits=31):
    """(node_pos uint32[N + 1], pos_bits, a_sat, key int64[N]) of the self-addressed CSR; None where the graph gets none."""
    deg = np.diff(np.asarray(indptr, np.int64))
    units = np.maximum(1, (deg + 31) >> 5)
    node_pos = np.zeros(len(deg) + 1, np.int64)
    np.cumsum(units, out=node_pos[1:])
    total = int(node_pos[-1])
    pos_bits = 1
    while pos_bits < 31 and (1 << pos_bits) < total + 1:
        pos_bits += 1
    spare = min(31 - pos_bits, max_degree_bits)
    if total == 0 or total >= (1 << 26) or spare < 2:
        return None
    a_sat = (1 << spare) - 1
    key = node_pos[:-1] | (np.minimum(deg, a_sat) << pos_bits)
    return node_pos.astype(np.uint32), pos_bits, a_sat, key


def acsr_row_words(indptr, indices, layout, node):
    """The column words of `node`'s row in the self-addressed CSR, padding included (units * 32 words)."""
    node_pos, _, _, key = layout
    lo, hi = int(indptr[node]), int(indptr[node + 1])
    n_units = int(node_pos[node + 1]) - int(node_pos[node])
    words = np.full(32 * n_units, -1, np.int32)
    words[:hi - lo] = key[indices[lo:hi]].astype(np.int32)
    return words


def packed_layout(indptr, max_degree_bits=31):
    """(id_bits, deg_sat, key int64[N]) of the packed CSR (deg_sat 0: plain column ids)."""
    deg = np.diff(np.asarray(indptr, np.int64))
    n = len(deg)
    id_bits = 1
    while id_bits < 31 and (1 << id_bits) < n:
        id_bits += 1
    spare = min(31 - id_bits, max_degree_bits)
    if spare < 2 or indptr[-1] == 0:
        return id_bits, 0, np.arange(n, dtype=np.int64)
    sat = (1 << spare) - 1
    return id_bits, sat, np.arange(n, dtype=np.int64) | (np.minimum(deg, sat) << id_bits)


# ------------------------------------------------------------------ the cases

N_NODES = 393216          # the smallest multiple of 65 536 at which all three families hold SET_SIZE keys below their window (smallest_n)
GRAPH_SEED = 20260
SET_SIZE = 64
HUB_LEN = 512
# Largest capacity a targeted table can have.  Sketch kernel, 768 threads: exact table CX = 2 964 slots, TOP-K's aggregation table
# (4 * 8192 + 12 * 2964 - 16 * (256 + 32)) / 12 = 5 310 slots at K = 32.  General kernel in its three-per-CU shape (512 threads,
# 53 248 bytes of LDS): (53248 - 5376) / 12 = 3 988 slots.
CAP_MAX = {"sk": 5312, "ga": 3988, "gp": 3988}
# ... and the capacities the control sets keep their homes apart at: the one-wave table (a set of 64: 4 x 64 < kMinCap), the full
# tables of both geometries; for the hub's 512 targets 4 x 512 slots and the full tables
CTL_CAPS = {"sk": (1024, 1172, 1940, 2960, 2964), "ga": (1024, 3988), "gp": (1024, 3988)}
HUB_CAPS = {"sk": (2048, 1940, 2960, 2964), "ga": (2048, 3988), "gp": (2048, 3988)}
FAMILIES = ("sk", "ga", "gp")
ROLES = ("A", "B", "m", "C", "hub")
PINNED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "collision_sets.json")


def window(family):
    return 65536 // (CAP_MAX[family] - K_PROBE_SPAN)


def hash16(family, key):
    return sk_hash16(key) if family == "sk" else hash_a(key) >> np.uint64(16)


def home(family, key, cap):
    return sk_home(key, cap) if family == "sk" else home_lds(key, cap)


def family_keys(family, indptr):
    return packed_layout(indptr)[2] if family == "gp" else acsr_layout(indptr)[3]


def _special_nodes(n, rng):
    """30 special node ids: family x (adversarial, control) x role."""
    ids = np.sort(rng.choice(np.arange(n // 4, 3 * n // 4), size=len(FAMILIES) * 2 * len(ROLES), replace=False))
    out, i = {}, 0
    for fam in FAMILIES:
        for kind in ("adv", "ctl"):
            for role in ROLES:
                out[(fam, kind, role)] = int(ids[i]); i += 1
    return out


_ROW_LEN = {"A": SET_SIZE, "B": 1, "m": SET_SIZE, "C": 1, "hub": HUB_LEN}


def _base(n, seed):
    """indptr, the ring rows as an (N, 4) id matrix + mask, and the special nodes -- everything the layout depends on."""
    rng = np.random.default_rng(seed)
    ring = rng.choice(np.array([0, 1, 3]), size=n)             # degrees 1, 2, 4: every share is a power of two
    special = _special_nodes(n, rng)
    deg = 1 + ring
    for (fam, kind, role), v in special.items():
        deg[v] = _ROW_LEN[role]
    indptr = np.zeros(n + 1, np.int32)
    np.cumsum(deg, out=indptr[1:])
    return rng, ring, special, indptr


def _select_sets(n, ring, special, indptr):
    """Per family: the collision set (the SET_SIZE smallest node ids below the window; None if there are fewer), the control
    set, the hub fillers of both."""
    is_special = np.zeros(n, bool)
    is_special[list(special.values())] = True
    sets = {}
    for fam in FAMILIES:
        key = family_keys(fam, indptr)
        cand = np.flatnonzero((hash16(fam, key) < window(fam)) & ~is_special)
        adv = cand[:SET_SIZE] if len(cand) >= SET_SIZE else None
        # control + fillers: walk the nodes in id order, keep those whose home is new at every capacity in play (and not slot 0's
        # neighbourhood, where the adversarial set probes)
        def distinct(caps, count, start, skip):
            homes = np.stack([home(fam, key, c) for c in caps]).astype(np.int64)
            ok = ~is_special & np.all(homes >= K_PROBE_SPAN, axis=0)
            ok[skip] = False
            used = [set() for _ in caps]
            out = []
            for v in np.flatnonzero(ok):
                if v < start or any(int(homes[j, v]) in used[j] for j in range(len(caps))):
                    continue
                for j in range(len(caps)):
                    used[j].add(int(homes[j, v]))
                out.append(int(v))
                if len(out) == count:
                    break
            assert len(out) == count, (fam, caps, len(out))
            return np.array(out, np.int64)
        if adv is None:
            sets[fam] = dict(adv=None, n_candidates=len(cand))
            continue
        ctl = distinct(CTL_CAPS[fam], SET_SIZE, n // 8, adv)
        hub_ctl = distinct(HUB_CAPS[fam], HUB_LEN, n // 8, adv)
        # the adversarial hub: the set + fillers with distinct homes that are not members
        fill = distinct(HUB_CAPS[fam], HUB_LEN - SET_SIZE, n // 2, adv)
        sets[fam] = dict(adv=adv, ctl=ctl, hub_adv=np.sort(np.concatenate([adv, fill])), hub_ctl=hub_ctl, n_candidates=len(cand))
    return sets


def smallest_n(seed=GRAPH_SEED, step=65536, limit=1 << 21):
    """The smallest multiple of `step` nodes at which every family's search finds its set (how N_NODES was chosen)."""
    for n in range(step, limit + 1, step):
        _, ring, special, indptr = _base(n, seed)
        is_special = np.zeros(n, bool); is_special[list(special.values())] = True
        if all(np.count_nonzero((hash16(f, family_keys(f, indptr)) < window(f)) & ~is_special) >= SET_SIZE for f in FAMILIES):
            return n
    return None


class Cases:
    """indptr / indices of the graph; special[(family, kind, role)] -> node; sets[family] -> member arrays; seeds(family, kind)."""

    def __init__(self, n=N_NODES, seed=GRAPH_SEED):
        self.n = n
        rng, ring, special, indptr = _base(n, seed)
        self.special, self.indptr = special, indptr
        self.sets = _select_sets(n, ring, special, indptr)
        for fam in FAMILIES:
            if self.sets[fam]["adv"] is None:
                raise ValueError(f"family {fam}: only {self.sets[fam]['n_candidates']} keys below the window at N = {n}")
        ids = (np.arange(n, dtype=np.int64)[:, None] + np.arange(4)[None, :]) % n
        keep = np.arange(4)[None, :] <= ring[:, None]
        ids = np.where(keep, ids, np.int64(1) << 40)
        ids.sort(axis=1)                                     # (rows hold strictly increasing ids, the wrap-around rows too)
        indices = np.empty(int(indptr[-1]), np.int32)
        normal = np.ones(n, bool); normal[list(special.values())] = False
        first = np.arange(4)[None, :] < (1 + ring)[:, None]  # after the sort the kept ids stand first
        rows_of = np.repeat(np.arange(n), np.diff(indptr))
        indices[normal[rows_of]] = ids[normal][first[normal]].astype(np.int32)
        for (fam, kind, role), v in special.items():
            s = self.sets[fam]
            row = {"A": s[kind], "m": s[kind], "hub": s["hub_" + kind],
                   "B": np.array([special[(fam, kind, "m")]]), "C": np.array([special[(fam, kind, "hub")]])}[role]
            assert len(row) == _ROW_LEN[role]
            indices[indptr[v]:indptr[v + 1]] = np.sort(row)
        self.indices = indices

    def seed(self, family, kind, which):
        return self.special[(family, kind, which)]

    def seeds(self, family, kind, which="ABC"):
        return np.array([self.special[(family, kind, w)] for w in which], np.int64)

    def members(self, family, kind):
        return self.sets[family][kind]

    def pinned(self):
        """What tests/golden/collision_sets.json records of these cases."""
        return {"n_nodes": self.n, "graph_seed": GRAPH_SEED,
                "special": {"/".join(k): v for k, v in self.special.items()},
                "sets": {f: {k: self.sets[f][k].tolist() for k in ("adv", "ctl")} for f in FAMILIES},
                "candidates": {f: self.sets[f]["n_candidates"] for f in FAMILIES}}


@functools.lru_cache(maxsize=1)
def cases():
    return Cases()


def load_pinned():
    with open(PINNED) as f:
        return json.load(f)


# the recipe of every collision test: four levels (level 3 is the last and only records), K = 32, every member of a set pushes.
# Coefficients, degrees and row lengths are powers of two, so every share and every sum of shares is exact in fp64 whatever the
# order of the adds: rows are the same BITS under every option, and equal totals are exact ties (ranked by column id).
COEF = np.array([0.5, 0.25, 0.125, 0.125])
RMAX = 1e-5
TOP_K = 32
