"""Cases, the order contract as a numpy float32 walk, and the deliberate mistakes of MAG's deterministic table gradient with
input dropout (csrc/mag_drop_abi.hpp), built on tests/mag_cases.py and tests/mag_det_cases.py.
tests/test_host_mag_drop.py audits them on the CPU, tests/test_gpu_mag_drop.py runs them on the GPU.

`walk_dW32_drop` is what gp_mag_prop_rows_backward_det_drop must give BIT FOR BIT: the per-sample slot gradient U[s, e, :],
per entry the samples' (U[s, e] * d) * m_in summed s ascending from 0.0f with the dropped samples passed over, per table row
the entries in entry order -- left to right, or with a chunk by gather_chunk_cases.chunked_sum.  The float64 reference of
the gradient is mag_cases.ref64.  Everything here runs on the CPU and is computed once per case.
"""
import functools

import numpy as np
import torch

import gather_chunk_cases as gcc
import mag_cases as mc
import mag_det_cases as dc
from grand_plus_amd._common import mag_slot_seed

f32 = np.float32
SEED = mc.SEED
CHUNK = 64

# a deliberate mistake -> what a kernel that made it would compute
MISTAKES = ("sample 0's mask for every sample", "keep_scale missing", "the batch slot in the seed", "h * n_t + t for t * H + h",
            "samples summed before the mask", "a dropped sample's seed reused")


def sample_weights32(P, batch, S, p_node, training, keep):
    """(w float32 [S, B * K], inv float32 [S, B], node int64 [B * K]): w'_{s,k} of every slot as stage_row has it (0 for a slot
    that does not exist), inv_{s,b} = 1 / (sum_k w' + 1e-12) summed sequentially in k, and the slot's node (-1: none)."""
    rows = P.rows(batch).numpy()
    K, B = P.K, len(rows)
    col, val = P.col.reshape(-1).numpy(), P.val.reshape(-1).numpy()
    scale = f32(1.0) / (f32(1.0) - f32(p_node)) if p_node < 1.0 else f32(0.0)
    km = None if keep is None else keep.reshape(S, -1).numpy()
    w, inv, node = np.zeros((S, B * K), f32), np.zeros((S, B), f32), np.full(B * K, -1, np.int64)
    for b, r in enumerate(rows):
        if not 0 <= r < P.S_rows:
            continue
        n = K if P.filled is None else max(0, min(int(P.filled[r]), K))
        for k in range(n):
            c = int(col[r * K + k])
            if not 0 <= c < P.N:
                continue
            node[b * K + k] = c
            x = np.full(S, f32(val[r * K + k]), f32)
            if training:
                x = x * np.where(km[:, r * K + k] != 0, scale, f32(0.0)).astype(f32)
            w[:, b * K + k] = x
        for s in range(S):
            den = f32(0.0)
            for k in range(n):
                den = den + w[s, b * K + k]
            inv[s, b] = f32(1.0) / (den + f32(1e-12))
    return w, inv, node


def slot_grads32_samples(P, batch, S, G, w, inv, node):
    """U float32 [S, B * K, H] of the order contract: ((g[s, b] * inv_{s,b}) * w'_{s,k}) * inv_den_n, 0 where w'_{s,k} == 0."""
    K, H = P.K, P.H
    indptr, data = P.indptr.numpy(), P.data.numpy()
    g = G.numpy().astype(f32)
    U = np.zeros((S, w.shape[1], H), f32)
    for e in np.flatnonzero(node >= 0):
        if not w[:, e].any():
            continue
        den = f32(0.0)
        for x in data[indptr[node[e]]:indptr[node[e] + 1]]:
            den = den + x
        inv_den = f32(1.0) / (den + f32(1e-10))
        b = e // K
        for s in range(S):
            if w[s, e] != 0.0:
                U[s, e] = ((g[s, b] * inv[s, b]) * w[s, e]) * inv_den
    return U


def _mask(seed, s, slot, n_t, H, p_in, transposed=False):
    """m_in of (sample s, slot): bool [n_t, H], element (t, h) keyed t * H + h (mag_cases.input_keep), or, for the mistake,
    h * n_t + t."""
    if not transposed:
        return mc.input_keep(seed, s, slot, n_t, H, p_in)
    return mc.hash_keep(mag_slot_seed(seed, s, int(slot)), np.arange(n_t * H), p_in).reshape(H, n_t).T


def entry_terms32(P, batch, S, p_node, p_in, training, keep, G, seed, mut=None, want_overlap=False):
    """(E, x): the entry order of mag_det_cases and x float32 [total, H], what every entry contributes to its table row by
    the contract (mut None) or under one of MISTAKES.  want_overlap: also whether some (entry, h) takes terms of two samples
    whose masks differ there."""
    assert mut is None or mut in MISTAKES, mut
    E = dc.entry_order(P, batch)
    w, inv, node = sample_weights32(P, batch, S, p_node, training, keep)
    U = slot_grads32_samples(P, batch, S, G, w, inv, node)
    rows = P.rows(batch).numpy()
    K, H = P.K, P.H
    d = E["d"].astype(f32)
    drop = training and p_in > 0.0
    scale_in = f32(1.0) / (f32(1.0) - f32(p_in)) if p_in < 1.0 else f32(0.0)
    if mut == "keep_scale missing" and p_in < 1.0:
        scale_in = f32(1.0)
    lens = np.diff(E["slot_base"])
    x = np.zeros((E["total"], H), f32)
    masks, overlap = {}, False
    if mut == "samples summed before the mask":                   # today's single U per slot, then one mask
        Usum = np.zeros(U.shape[1:], f32)
        for s in range(S):
            Usum = Usum + U[s]
    for e in np.flatnonzero(lens > 0):
        j0, n_t = int(E["slot_base"][e]), int(lens[e])
        b, k = divmod(int(e), K)
        rslot = int(rows[b]) * K + k
        live = [s for s in range(S) if w[s, e] != 0.0]
        xe = np.zeros((n_t, H), f32)
        seen = []
        for rank, s in enumerate(live):
            m = np.ones((n_t, H), bool)
            if drop:
                ms = 0 if mut == "sample 0's mask for every sample" else rank if mut == "a dropped sample's seed reused" else s
                key = (ms, e if mut == "the batch slot in the seed" else rslot, n_t)
                if key not in masks:
                    masks[key] = _mask(seed, key[0], key[1], n_t, H, p_in, mut == "h * n_t + t for t * H + h")
                m = masks[key]
            if mut == "samples summed before the mask":
                if rank == 0:
                    xe = xe + (Usum[e][None, :] * d[j0:j0 + n_t, None]) * np.where(m, scale_in, f32(0.0)).astype(f32)
                continue
            xe = xe + (U[s, e][None, :] * d[j0:j0 + n_t, None]) * (np.where(m, scale_in, f32(0.0)).astype(f32) if drop else f32(1.0))
            if want_overlap and not overlap:
                nz = U[s, e] != 0.0
                overlap = any(bool(((m != m2) & nz[None, :] & nz2[None, :]).any()) for m2, nz2 in seen)
                seen.append((m, nz))
        x[j0:j0 + n_t] = xe
    return (E, x, overlap) if want_overlap else (E, x)


def walk_dW32_drop(P, batch, S, p_node, p_in, training, keep, G, seed, max_entries=None, chunk=None, mut=None):
    """dW float32 [V, H] by the order contract of mag_drop_abi.hpp: the entries below max_entries (when given), sorted by a
    stable sort of their keys, summed per table row left to right from 0.0f, or in chunks of `chunk` sorted positions."""
    E, x = entry_terms32(P, batch, S, p_node, p_in, training, keep, G, seed, mut)
    n = E["total"] if max_entries is None else min(E["total"], max_entries)
    keys = E["keys"][:n]
    order = np.argsort(keys, kind="stable")
    sk, terms = keys[order], x[:n][order]
    dW = gcc.left_to_right(sk, terms, P.V) if chunk is None else gcc.chunked_sum(sk, terms, P.V, chunk)
    return torch.from_numpy(dW)


# ---- the cases
#     name              where it comes from                       what it is there for
CASES = ("pin05_h65_s3", "pin05_h64_k32", "pin05_s16", "pin1", "eps_scale",       # mag_cases.CASES with input dropout
         "h257_k5_s2",                                                             # H > 256: a second column pass of the gather
         "k1024_s16",                                                              # H = 1: the weight rows take two LDS stages
         "segments",                                                               # segments of 63, 64 and 65 entries, one past its window
         "bad_indices",                                                            # ids, columns and batch rows out of range
         "hub")                                                                    # 4 097 entries on one table row
DEGENERATE = ("pin1",)                                                             # input_droprate = 1: every mask is all zero
P_IN = 0.5


def _problem(name):
    """(P, batch, S, p_node, p_in, training, keep for the walk, keep for the call, G)."""
    if name in mc.CASES and name != "hub":                                          # mag_cases' hub has no input dropout
        c = mc.case(name)
        kw = c["kw"]
        return c["P"], c["batch"], c["S"], kw["dropnode_rate"], kw["input_droprate"], kw["training"], c["keep"], c["keep"], c["G"]
    if name in dc.WALKS:
        c = dc.walk_case(name)
        H, K, S, _filled, _mode, p_node, training, mask = dc.WALKS[name]
        P = c["P"]
        call_keep = c["kw"]["keep"]
        keep = call_keep if mask == "explicit" else mc.node_keep(SEED, S, P.S_rows * K, p_node)
        return P, c["batch"], S, p_node, P_IN, training, keep, call_keep, c["G"]
    if name == "segments":
        P, S = dc.segments_problem(), 2
        keep = torch.ones((S, 4), dtype=torch.uint8)
        keep[1, 2] = 0                                                              # one slot dropped in one sample
        G = torch.randn((S, 2, P.H), generator=torch.Generator().manual_seed(3))
        return P, None, S, 0.5, P_IN, True, keep, keep, G
    assert name == "hub"
    P, S = mc.problem(7, 1, bags=(3, 2, 1, 4097), filled="full", S_rows=2), 2
    assert P.longest == 4097
    keep = torch.ones((S, 2), dtype=torch.uint8)
    G = torch.randn((S, 2, P.H), generator=torch.Generator().manual_seed(11))
    return P, None, S, 0.0, P_IN, True, keep, keep, G


@functools.lru_cache(maxsize=None)
def case(name):
    """One case, computed once: the problem P, the batch, mag_prop_rows' keywords, G, S, the explicit DropNode mask the walk
    uses (`keep`: the hashed one rebuilt on the host where the call hashes it), the entry order E, the float32 walks of the
    contract unchunked and in chunks of CHUNK, and whether two samples' masks differ on a common element."""
    P, batch, S, p_node, p_in, training, keep, call_keep, G = _problem(name)
    kw = dict(samples=S, dropnode_rate=p_node, input_droprate=p_in, training=training, seed=SEED, keep=call_keep)
    E, _x, overlap = entry_terms32(P, batch, S, p_node, p_in, training, keep, G, SEED, want_overlap=True)
    args = (P, batch, S, p_node, p_in, training, keep, G, SEED)
    return {"P": P, "batch": batch, "kw": kw, "G": G, "S": S, "keep": keep, "E": E, "args": args, "overlap": overlap,
            "dW": walk_dW32_drop(*args), "dW_chunked": walk_dW32_drop(*args, chunk=CHUNK)}


def _reference_problem(P, batch, G):
    """An equal problem that the float64 chain can index: an attribute id out of range names a zero row appended to the
    table (its weight still counts in the bag's denominator, as in the kernel), a column out of range becomes node 0 with the
    score 0 (weight 0: absent), and a batch row out of range becomes row 0 with a zero upstream gradient."""
    Q = mc.Problem(**P.__dict__)
    Q.indices, Q.col, Q.val = P.indices.clone(), P.col.clone(), P.val.clone()
    bad_a = (Q.indices < 0) | (Q.indices >= P.V)
    Q.indices[bad_a] = P.V
    Q.W = torch.cat([P.W, torch.zeros((1, P.H))])
    Q.V = P.V + 1
    bad_c = (Q.col < 0) | (Q.col >= P.N)
    Q.col[bad_c], Q.val[bad_c] = 0, 0.0
    G = G.clone()
    if batch is not None:
        batch = batch.clone()
        bad_b = (batch < 0) | (batch >= P.S_rows)
        batch[bad_b] = 0
        G[:, bad_b] = 0.0
    return Q, batch, G


@functools.lru_cache(maxsize=None)
def reference(name):
    """(dW64, dW_terms, n): mag_cases.ref64's gradient and its sum of magnitudes, [V, H] each, and n [V, 1], the number of
    roundings the bound stands for: S terms per contribution, the longest bag and S."""
    c = case(name)
    P, batch, S, p_node, p_in, training, keep, G, seed = c["args"]
    Q, qbatch, QG = _reference_problem(P, batch, G)
    _out, _terms, dW64, dW_terms = mc.ref64(Q, qbatch, S, p_node, p_in, training, keep, seed, QG)
    n = S * dc.contributions(P, batch).double()[:, None] + P.longest + S
    return dW64[:P.V], dW_terms[:P.V], n


def bound(name):
    """test_gpu_mag_det.py's derived bound with n = S * contributions + the longest bag + S: every entry now adds up to S
    products to its destination's sequential sum."""
    _dW64, dW_terms, n = reference(name)
    return (n + 8) * 2.0 ** -24 * dW_terms + 1e-7
