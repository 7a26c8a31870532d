"""Inputs and references shared by tests/test_host_mag_det.py and tests/test_gpu_mag_det.py, built on
tests/mag_cases.py.

`entry_order` is the brute-force enumeration of a call's entries in the order (b, k, t) with their keys: what
gp_mag_det_keys must write and csrc/mag_det_layout.hpp must search.  `walk_dW32` is a numpy float32 walk of the order
contract of csrc/mag_det_abi.hpp: what the deterministic backward must give BIT FOR BIT.  The float64 reference of the
gradient is mag_cases.ref64.  Everything here runs on the CPU.
"""
import functools

import numpy as np
import torch

import mag_cases as mc

f32 = np.float32
GRID_BAGS = (0, 1, 63, 64, 65)
GRID = {1: (1, 1), 1023: (33, 31), 1024: (32, 32), 1025: (25, 41)}        # slot count -> (B, K): around the scan's 1 024
SLACK = (-1, 0, 130, 1000)                                                # max_entries - total; 1 000: four passes of a 256-thread tail


def grid_problem(n_slots):
    """A problem of exactly n_slots = B * K slots whose bags cycle through 0, 1, 63, 64, 65 entries; ragged rows from 2 rows on."""
    B, K = GRID[n_slots]
    return mc.problem(1, K, bags=GRID_BAGS, S_rows=B, filled="ragged" if B > 1 else None, seed=n_slots)


def entry_order(P, batch):
    """The entries of mag_prop_rows(P, batch_rows=batch) in the order (b, k, t): a dict with slot_base int64 [B * K + 1],
    total, and per entry slot (e = b * K + k), t, the raw attribute id a, the weight d and the key (a, or V for an id
    outside [0, V)).  A slot exists as mag_det_abi.hpp says; every other slot has no entry."""
    rows = P.rows(batch).numpy()
    K, B = P.K, len(rows)
    col, indptr = P.col.reshape(-1).numpy(), P.indptr.numpy()
    lens, node = np.zeros(B * K, np.int64), np.full(B * K, -1, np.int64)
    for b, r in enumerate(rows):
        if not 0 <= r < P.S_rows:
            continue
        n = K if P.filled is None else min(int(P.filled[r]), K)
        for k in range(max(n, 0)):
            c = int(col[r * K + k])
            if 0 <= c < P.N:
                node[b * K + k] = c
                lens[b * K + k] = max(int(indptr[c + 1] - indptr[c]), 0)
    base = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    slot = np.repeat(np.arange(B * K), lens)
    t = np.arange(int(base[-1])) - base[slot]
    pos = indptr[node[slot]] + t
    a = P.indices.numpy()[pos].astype(np.int64)
    return {"slot_base": base, "total": int(base[-1]), "slot": slot, "t": t, "a": a, "d": P.data.numpy()[pos],
            "keys": np.where((a >= 0) & (a < P.V), a, P.V), "node": node}


def slot_grads32(P, batch, S, p_node, training, keep, G):
    """U float32 [B * K, H] of the order contract: c_e = sum_s (g[s, b] * inv_{s,b}) * w'_{s,k} (s ascending, from 0.0f)
    times the bag's 1 / (sum_t d_t + 1e-10), both denominators summed sequentially; 0 for a slot dropped in every sample."""
    rows = P.rows(batch).numpy()
    K, H, B = P.K, P.H, len(rows)
    col, val = P.col.reshape(-1).numpy(), P.val.reshape(-1).numpy()
    indptr, data = P.indptr.numpy(), P.data.numpy()
    g = G.numpy().astype(f32)
    scale = f32(1.0) / (f32(1.0) - f32(p_node)) if p_node < 1.0 else f32(0.0)
    km = None if keep is None else keep.reshape(S, -1).numpy()
    U = np.zeros((B * K, H), f32)
    for b, r in enumerate(rows):
        if not 0 <= r < P.S_rows:
            continue
        n = K if P.filled is None else max(0, min(int(P.filled[r]), K))
        ok = [0 <= int(col[r * K + k]) < P.N for k in range(n)]
        w = np.zeros((S, n), f32)
        for s in range(S):
            for k in range(n):
                x = f32(val[r * K + k])
                if training:
                    x = x * (scale if km[s, r * K + k] else f32(0.0))
                w[s, k] = x if ok[k] else f32(0.0)
        inv = np.zeros(S, f32)
        for s in range(S):
            den = f32(0.0)
            for k in range(n):
                den = den + w[s, k]
            inv[s] = f32(1.0) / (den + f32(1e-12))
        for k in range(n):
            if not ok[k] or not w[:, k].any():
                continue
            c = np.zeros(H, f32)
            for s in range(S):
                c = c + (g[s, b] * inv[s]) * w[s, k]
            node = int(col[r * K + k])
            den = f32(0.0)
            for x in data[indptr[node]:indptr[node + 1]]:
                den = den + x
            U[b * K + k] = c * (f32(1.0) / (den + f32(1e-10)))
    return U


def walk_dW32(P, batch, S, p_node, training, keep, G, max_entries=None):
    """dW float32 [V, H] by the order contract: for every entry j ascending (below max_entries, when given),
    dW[a_j] = dW[a_j] + U[e_j] * d_j from zeros, ids outside [0, V) passed over."""
    E = entry_order(P, batch)
    U = slot_grads32(P, batch, S, p_node, training, keep, G)
    dW = np.zeros((P.V, P.H), f32)
    n = E["total"] if max_entries is None else min(E["total"], max_entries)
    for j in range(n):
        a = int(E["a"][j])
        if 0 <= a < P.V:
            dW[a] = dW[a] + U[E["slot"][j]] * E["d"][j]
    return torch.from_numpy(dW)


def contributions(P, batch):
    """How many entries name each table row: int64 [V]."""
    E = entry_order(P, batch)
    a = E["a"][(E["a"] >= 0) & (E["a"] < P.V)]
    return torch.from_numpy(np.bincount(a, minlength=P.V).astype(np.int64))


def with_bad_indices(P):
    """A copy of P with an attribute id, a column and (through `BAD_BATCH`) batch rows out of range on both sides."""
    Q = mc.Problem(**P.__dict__)
    Q.indices, Q.col = P.indices.clone(), P.col.clone()
    nz = int(P.indptr[4])                                                  # inside node 3's bag, which every row holds
    Q.indices[nz - 1], Q.indices[nz - 2] = P.V + 3, -1
    Q.col[2, 1], Q.col[3, 0] = P.N + 2, -1
    return Q


def bad_batch(S_rows):
    return torch.tensor([2, S_rows + 1, 3, -1, 1], dtype=torch.int32)


#        name          H    K   S  filled    batch       p_node training mask
WALKS = {
    "h1_k1_s1":      (1,   1,  1,  "full",   None,       0.5,   True,   "explicit"),
    "h7_k5_s3":      (7,   5,  3,  "ragged", "reversed", 0.5,   True,   "explicit"),
    "h64_k32_s2":    (64,  32, 2,  "ragged", "repeat",   0.5,   True,   "hash"),
    "h65_k5_s16":    (65,  5,  16, None,     None,       0.5,   True,   "explicit"),
    "h257_k5_s2":    (257, 5,  2,  "ragged", "repeat",   0.5,   True,   "hash"),
    "k32_full_s3":   (7,   32, 3,  "full",   "reversed", 0.5,   True,   "hash"),
    "filled0":       (7,   5,  2,  "zero",   None,       0.5,   True,   "explicit"),
    "eval":          (64,  5,  1,  "ragged", None,       0.5,   False,  None),
    "pnode1":        (7,   5,  2,  "ragged", None,       1.0,   True,   "explicit"),
    "bad_indices":   (7,   5,  3,  "full",   "bad",      0.5,   True,   "explicit"),
    "k1024_s16":     (1,   1024, 16, "ragged", None,     0.5,   True,   "hash"),   # the 16 weight rows take two LDS stages
}
S_ROWS = {"k1024_s16": 3}
SEED = mc.SEED


@functools.lru_cache(maxsize=None)
def walk_case(name):
    """One case of WALKS, computed once: the problem P, the batch, mag_prop_rows' keywords (with the explicit mask or the
    seed of the hashed one), G, the entry order and the float32 walk of the contract."""
    H, K, S, filled, mode, p_node, training, mask = WALKS[name]
    bags = mc.BAGS if K <= 5 else mc.BAGS[:5]
    P = mc.problem(H, K, bags=bags, filled="full" if filled == "zero" else filled, S_rows=S_ROWS.get(name, 6))
    if filled == "zero":
        P.filled = torch.zeros(P.S_rows, dtype=torch.int32)
    if mode == "bad":
        P, batch = with_bad_indices(P), bad_batch(P.S_rows)
    else:
        batch = mc.batch_rows(mode, P.S_rows)
    g = torch.Generator().manual_seed(len(name) + 31 * H)
    L = P.S_rows * K
    if not training:
        keep = None
    elif mask == "explicit":
        keep = (torch.rand((S, L), generator=g) >= p_node).to(torch.uint8)
    else:
        keep = mc.node_keep(SEED, S, L, p_node)
    B = P.S_rows if batch is None else batch.numel()
    G = torch.randn((S, B, H), generator=g)
    kw = dict(samples=S, dropnode_rate=p_node, input_droprate=0.0, training=training, seed=SEED,
              keep=keep if mask == "explicit" else None)
    E = entry_order(P, batch)
    return {"P": P, "batch": batch, "kw": kw, "G": G, "S": S, "E": E, "dW": walk_dW32(P, batch, S, p_node, training, keep, G)}


def segments_problem():
    """Single-attribute bags of 65, 63, 64 and 64 entries (attributes 2, 0, 3, 1) met in that entry order, so that the
    sorted list holds segments of 63, 64, 65 and 64 entries: attribute 1's starts at sorted position 63 and runs past its
    window, attribute 2's starts at 127."""
    lens, attr = [65, 63, 64, 64], [2, 0, 3, 1]
    g = torch.Generator().manual_seed(5)
    indptr = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64)
    indices = torch.cat([torch.full((n,), a, dtype=torch.int32) for n, a in zip(lens, attr)])
    data = torch.rand(int(indptr[-1]), generator=g) + 0.05
    col = torch.tensor([[0, 1], [2, 3]], dtype=torch.int32)
    val = torch.rand((2, 2), generator=g, dtype=torch.float64) + 0.1
    return mc.Problem(W=torch.randn((5, 65), generator=g), indptr=indptr, indices=indices, data=data, col=col, val=val, filled=None,
                      K=2, N=4, V=5, H=65, S_rows=2, longest=65)


def order_pin_problem(n=8):
    """H = 1, eval mode, K = 1, n rows of weight 1 whose nodes hold the one attribute 0 with d = 1: U[e] = g[b] exactly
    (every denominator rounds to 1), so dW[0] is the float32 left-to-right sum of g."""
    indptr = torch.arange(n + 1, dtype=torch.int64)
    P = mc.Problem(W=torch.zeros((2, 1)), indptr=indptr, indices=torch.zeros(n, dtype=torch.int32), data=torch.ones(n),
                   col=torch.arange(n, dtype=torch.int32).reshape(n, 1), val=torch.ones((n, 1), dtype=torch.float64), filled=None,
                   K=1, N=n, V=2, H=1, S_rows=n, longest=1)
    G = torch.tensor([2.0 ** 25, 1.0, -2.0 ** 25, 1.0] * (n // 4)).reshape(1, n, 1)
    return P, G
