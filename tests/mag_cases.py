"""Inputs, references and bounds shared by tests/test_gpu_mag_rows.py and tests/test_host_mag_rows.py.

The reference is a float64 restatement of the two formulas of grandplus_mag.h with explicit masks (`ref64`: MLP.emb of
model_mag.py:48-55 per slot occurrence, then oracle.random_prop_ref), with gradients by float64 autograd; `emulate` is a
float32 numpy walk of the order contract (what the kernel must give bit for bit is NOT asserted from it: it shows that
the contract's own rounding stays inside the tolerance).  `hash_keep` mirrors the device's counter hash, so both masks
of a hashed call can be rebuilt on the host.  Everything here runs on the CPU and is computed once per case.

Tolerance: §7d's rule (augment_cases.close), |d| <= 1e-5 * sum|terms| + 1e-7 with sum|terms| the nested sum of absolute
products.  An output element is reached through at most (slots + longest bag + S + 8) fp32 roundings of relative size
2^-24 each on a sum of non-negative magnitudes -- the slot sum, the bag sum, the two denominators and their reciprocals,
the products; every case is sized so that this count is at most 160, and 160 * 2^-24 < 1e-5.  The hub case (one bag of
4 097 entries) takes §7i's derived bound (n + 8) * 2^-24 * sum|terms| + 1e-7 with n = slots + longest bag + S."""
import functools

import numpy as np
import torch

from grand_plus_amd._common import mag_slot_seed, sample_seed
from oracle.random_prop_ref import random_prop_ref

BAGS = (0, 1, 63, 64, 65, 130)
ROUNDINGS = 160


def hash_keep(seed, entries, p):
    """keep_scale of csrc/gp_common.hpp on the host: True where entry e of `seed` is kept at rate p."""
    e = np.asarray(entries, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = np.uint64(seed) + e * np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    u = (x >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return u >= np.float32(p)


def node_keep(seed, S, L, p):
    """The hashed DropNode mask of an S-sample call over L = S_rows * K entries: uint8 [S, L] (random_prop_rows's too)."""
    return torch.from_numpy(np.stack([hash_keep(sample_seed(seed, s), np.arange(L), p) for s in range(S)]).astype(np.uint8))


def input_keep(seed, s, e, n_t, H, p):
    """The hashed input-dropout mask of (sample s, slot e): bool [n_t, H], element (t, h) keyed t * H + h."""
    return hash_keep(mag_slot_seed(seed, s, int(e)), np.arange(n_t * H), p).reshape(n_t, H)


class Problem:
    """The CPU tensors of one problem, in the dtypes mag_prop_rows takes."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def cuda(self):
        t = lambda x: None if x is None else x.cuda()                       # noqa: E731
        return (t(self.W), t(self.indptr), t(self.indices), t(self.data), t(self.col.reshape(-1)), t(self.val.reshape(-1)),
                t(self.filled), self.K)

    def rows(self, batch):
        if batch is None:
            return torch.arange(self.S_rows)
        return batch.long()


def problem(H, K, bags=BAGS, S_rows=6, V=50, filled="ragged", seed=0):
    """Nodes whose bag lengths cycle through `bags` (node 3 has bags[3]), S_rows resident rows of K slots; node 3 sits in
    slot 0 of every row and twice in row 1.  filled: "ragged" (row 0 empty, row 1 full), "full" or None (no filled array: every slot filled)."""
    g = torch.Generator().manual_seed(seed * 100003 + H * 131 + K)
    N = 2 * len(bags)
    lens = torch.tensor([bags[i % len(bags)] for i in range(N)], dtype=torch.int64)
    indptr = torch.zeros(N + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(lens, 0)
    nnz = int(indptr[-1])
    indices = torch.randint(0, V, (nnz,), generator=g, dtype=torch.int32)
    data = torch.rand((nnz,), generator=g) + 0.05
    col = torch.randint(0, N, (S_rows, K), generator=g, dtype=torch.int32)
    col[:, 0] = 3
    if K > 1:
        col[1, K - 1] = 3
    val = torch.rand((S_rows, K), generator=g, dtype=torch.float64) ** 3 + 1e-9
    if filled == "ragged":
        f = torch.randint(0, K + 1, (S_rows,), generator=g, dtype=torch.int32)
        f[0], f[1] = 0, K
    elif filled == "full":
        f = torch.full((S_rows,), K, dtype=torch.int32)
    else:
        f = None
    W = torch.randn((V, H), generator=g)
    return Problem(W=W, indptr=indptr, indices=indices, data=data, col=col, val=val, filled=f, K=K, N=N, V=V, H=H,
                   S_rows=S_rows, longest=int(lens.max()))


def at_eps_scale(P):
    """Row 2's scores become 1e-13, so that the sum of the kept ones is of the size of the 1e-12 beside it, and the one
    attribute of node 1, which row 3 names in slot 1, gets the weight 5e-11, half of the 1e-10 beside it: there
    1 / (den + eps), 1 / den, 1 / max(den, eps) and the other formula's epsilon all differ by tens of per cent."""
    P.val[2, :] = 1e-13
    P.col[3, 1] = 1
    assert int(P.indptr[2] - P.indptr[1]) == 1
    P.data[int(P.indptr[1])] = 5e-11


def _entries(P, batch):
    """The filled slots of the batch, row after row: (idx = batch position, e = r * K + k, node)."""
    rows = P.rows(batch)
    n = torch.full((rows.numel(),), P.K, dtype=torch.int64) if P.filled is None else P.filled.long()[rows].clamp(0, P.K)
    sel = torch.arange(P.K)[None, :] < n[:, None]
    idx = torch.repeat_interleave(torch.arange(rows.numel()), n)
    e = (rows[:, None] * P.K + torch.arange(P.K)[None, :])[sel]
    return idx, e, P.col.reshape(-1)[e].long(), rows.numel()


def chain64(P, W, batch, S, p_node, p_in, training, keep, seed):
    """The two formulas of grandplus_mag.h on the table W (any float64 [V, H] tensor; differentiable): out [S, B, H].
    keep uint8 [S, S_rows * K] is the DropNode mask (None in eval mode); the input-dropout mask is the hashed one of `seed`."""
    idx, e, nodes, B = _entries(P, batch)
    M, H = e.numel(), P.H
    lens = P.indptr[nodes + 1] - P.indptr[nodes]
    occ = torch.repeat_interleave(torch.arange(M), lens)
    first = torch.cumsum(lens, 0) - lens
    t = torch.arange(int(lens.sum())) - first[occ]
    pos = P.indptr[nodes][occ] + t
    a, d = P.indices[pos].long(), P.data[pos].double()
    scores = P.val.reshape(-1)[e].float().double()                                # model_mag.py:343: float32 scores
    drop_in = training and p_in > 0.0
    scale_in = 1.0 / (1.0 - p_in) if p_in < 1.0 else 0.0
    outs = []
    for s in range(S):
        fe = W[a]                                                                 # model_mag.py:49
        if drop_in:                                                               # model_mag.py:50
            m = np.concatenate([input_keep(seed, s, e[j], int(lens[j]), H, p_in) for j in range(M)] + [np.zeros((0, H), bool)])
            fe = fe * torch.from_numpy(m).double() * scale_in
        num = torch.zeros((M, H), dtype=torch.float64).index_add_(0, occ, fe * d[:, None])
        den = torch.zeros((M, 1), dtype=torch.float64).index_add_(0, occ, d[:, None])
        emb = num / (den + 1e-10)                                                 # model_mag.py:51-54
        o = torch.zeros((B, H), dtype=torch.float64)
        if M:
            r = random_prop_ref(emb, scores, idx, p_node, training, None if keep is None else keep[s].reshape(-1)[e])
            o = torch.cat([r, o[r.shape[0]:]])                                    # trailing empty rows
        outs.append(o)
    return torch.stack(outs)


# ---- the two formulas written out, and one deliberate mistake (tests/test_host_mutants.py)
MUTANTS = ("den_no_eps", "den_eps_swapped", "den_max", "keep_scale_missing", "sample0_mask_for_all", "bag_not_normalised")


def divide(num, den, eps, other, mut):
    """num / (den + eps), or what a mistaken denominator gives: none, the other formula's epsilon, max(den, eps)."""
    if mut == "den_no_eps":
        return num / den
    if mut == "den_eps_swapped":
        return num / (den + other)
    if mut == "den_max":
        return num / den.clamp(min=eps)
    return num / (den + eps)


def manual64(P, batch, S, p_node, p_in, training, keep, seed, mut=None):
    """chain64 on P.W from explicit formulas (mut None), or with one of MUTANTS built in: out [S, B, H]."""
    idx, e, nodes, B = _entries(P, batch)
    M, H = e.numel(), P.H
    lens = P.indptr[nodes + 1] - P.indptr[nodes]
    occ = torch.repeat_interleave(torch.arange(M), lens)
    first = torch.cumsum(lens, 0) - lens
    pos = P.indptr[nodes][occ] + torch.arange(int(lens.sum())) - first[occ]
    a, d = P.indices[pos].long(), P.data[pos].double()
    scores = P.val.reshape(-1)[e].float().double()
    W = P.W.double()
    scaled = mut != "keep_scale_missing"
    scale_in = (1.0 / (1.0 - p_in) if p_in < 1.0 else 0.0) if scaled or p_in >= 1.0 else 1.0
    scale_node = (1.0 / (1.0 - p_node) if p_node < 1.0 else 0.0) if scaled or p_node >= 1.0 else 1.0
    out = torch.zeros((S, B, H), dtype=torch.float64)
    for s in range(S):
        sm = 0 if mut == "sample0_mask_for_all" else s
        fe = W[a]
        if training and p_in > 0.0:
            m = np.concatenate([input_keep(seed, sm, e[j], int(lens[j]), H, p_in) for j in range(M)] + [np.zeros((0, H), bool)])
            fe = fe * torch.from_numpy(m).double() * scale_in
        num = torch.zeros((M, H), dtype=torch.float64).index_add_(0, occ, fe * d[:, None])
        den = torch.zeros((M, 1), dtype=torch.float64).index_add_(0, occ, d[:, None])
        emb = num if mut == "bag_not_normalised" else divide(num, den, 1e-10, 1e-12, mut)
        w = scores * keep[sm].reshape(-1)[e].double() * scale_node if training else scores
        num2 = torch.zeros((B, H), dtype=torch.float64).index_add_(0, idx, emb * w[:, None])
        den2 = torch.zeros((B, 1), dtype=torch.float64).index_add_(0, idx, w[:, None])
        out[s] = divide(num2, den2, 1e-12, 1e-10, mut)
    return out


def ref64(P, batch, S, p_node, p_in, training, keep, seed, G=None):
    """(out, terms[, dW, dW_terms]) in float64: chain64 on P.W, and on magnitudes (terms).  With G [S, B, H]: the gradient
    of sum(out * G) with respect to W, and the same on magnitudes."""
    def run(W, Gs):
        out = chain64(P, W, batch, S, p_node, p_in, training, keep, seed)
        if Gs is None:
            return out, None
        return out, torch.autograd.grad((out * Gs).sum(), W, allow_unused=True)[0]

    W64 = P.W.double().requires_grad_(G is not None)
    Wa = P.W.double().abs().requires_grad_(G is not None)
    out, dW = run(W64, None if G is None else G.double())
    terms, dWa = run(Wa, None if G is None else G.double().abs())
    if G is None:
        return out.detach(), terms.detach()
    zero = torch.zeros_like(P.W, dtype=torch.float64)
    return out.detach(), terms.detach(), zero if dW is None else dW, zero if dWa is None else dWa


def n_waves(K):
    w = 1
    while w < K and w < 16:
        w *= 2
    return w


def emulate(P, batch, S, p_node, p_in, training, keep, seed):
    """The order contract of grandplus_mag.h walked in float32 numpy: out [S, B, H]."""
    f32 = np.float32
    rows = P.rows(batch).numpy()
    W, indptr, indices, data = P.W.numpy(), P.indptr.numpy(), P.indices.numpy(), P.data.numpy()
    col, val = P.col.reshape(-1).numpy(), P.val.reshape(-1).numpy()
    K, H, nw = P.K, P.H, n_waves(P.K)
    scale_node = f32(1.0) / (f32(1.0) - f32(p_node)) if p_node < 1.0 else f32(0.0)
    scale_in = f32(1.0) / (f32(1.0) - f32(p_in)) if p_in < 1.0 else f32(0.0)
    drop_in = training and p_in > 0.0
    out = np.zeros((S, len(rows), H), f32)
    for b, r in enumerate(rows):
        n = K if P.filled is None else max(0, min(int(P.filled[r]), K))
        for s in range(S):
            w = val[r * K:r * K + n].astype(f32)
            if training:
                w = w * np.where(keep[s].reshape(-1).numpy()[r * K:r * K + n] != 0, scale_node, f32(0.0)).astype(f32)
            den = f32(0.0)
            for k in range(n):
                den = den + w[k]
            total = np.zeros(H, f32)
            for wave in range(nw):
                acc = np.zeros(H, f32)
                for k in range(wave, n, nw):
                    if w[k] == 0.0:
                        continue
                    node = col[r * K + k]
                    lo, hi = indptr[node], indptr[node + 1]
                    m = input_keep(seed, s, r * K + k, hi - lo, H, p_in) if drop_in else None
                    e_acc, bden = np.zeros(H, f32), f32(0.0)
                    for t in range(hi - lo):
                        v = W[indices[lo + t]]
                        if drop_in:
                            v = v * np.where(m[t], scale_in, f32(0.0)).astype(f32)
                        e_acc = e_acc + v * data[lo + t]
                        bden = bden + data[lo + t]
                    acc = acc + w[k] * (e_acc * (f32(1.0) / (bden + f32(1e-10))))
                total = total + acc
            out[s, b] = total * (f32(1.0) / (den + f32(1e-12)))
    return torch.from_numpy(out)


def batch_rows(mode, S_rows):
    if mode is None:
        return None
    if mode == "reversed":
        return torch.arange(S_rows - 1, -1, -1, dtype=torch.int32)
    return torch.tensor([2, 0, 2, S_rows - 1, 1], dtype=torch.int32)               # "repeat": row 2 twice


#        name            H    K   S  filled    batch       p_node p_in  training  bags
CASES = {
    "h1_k1_s1":        (1,   1,  1,  "full",   None,       0.5,   0.0,  True,  BAGS),
    "h7_k5_s3":        (7,   5,  3,  "ragged", "reversed", 0.5,   0.0,  True,  BAGS),
    "h64_k32_s2":      (64,  32, 2,  "ragged", "repeat",   0.5,   0.0,  True,  BAGS[:5]),
    "h65_k5_s16":      (65,  5,  16, None,     None,       0.5,   0.0,  True,  BAGS),
    "h130_k32_s3":     (130, 32, 3,  "full",   "reversed", 0.5,   0.0,  True,  BAGS[:5]),
    "eval":            (64,  5,  1,  "ragged", None,       0.5,   0.5,  False, BAGS),
    "pnode0":          (7,   5,  2,  "ragged", "repeat",   0.0,   0.0,  True,  BAGS),
    "pnode1":          (7,   5,  2,  "ragged", None,       1.0,   0.0,  True,  BAGS),
    "pin05_h65_s3":    (65,  5,  3,  "ragged", "repeat",   0.5,   0.5,  True,  BAGS),
    "pin05_h64_k32":   (64,  32, 2,  "full",   None,       0.5,   0.5,  True,  BAGS[:5]),
    "pin05_s16":       (7,   5,  16, None,     "reversed", 0.5,   0.5,  True,  BAGS[:5]),
    "pin1":            (7,   5,  2,  "ragged", None,       0.5,   1.0,  True,  BAGS),
    "pin0_pnode0":     (64,  32, 1,  None,     None,       0.0,   0.0,  True,  BAGS[:5]),
    "hub":             (7,   1,  1,  "full",   None,       0.0,   0.0,  True,  (3, 2, 1, 4097)),
    # both denominators at the scale of their epsilons (see `at_eps_scale`)
    "eps_scale":       (7,   5,  2,  "full",   None,       0.5,   0.5,  True,  BAGS),
}
SEED = 0x5EED0FACADE


@functools.lru_cache(maxsize=None)
def case(name):
    """Everything a test needs of one case, computed once: a dict with the problem P, batch (int32 or None), the call's
    keywords, the explicit DropNode mask keep (None in eval mode), G, the float64 reference (out, terms, dW, dW_terms)
    and the number of roundings the tolerance stands for."""
    H, K, S, filled, mode, p_node, p_in, training, bags = CASES[name]
    P = problem(H, K, bags=bags, filled=filled, S_rows=2 if name == "hub" else 6)
    if name == "eps_scale":
        at_eps_scale(P)
    roundings = K + P.longest + S + 8
    assert name == "hub" or roundings <= ROUNDINGS, (name, roundings)
    batch = batch_rows(mode, P.S_rows)
    g = torch.Generator().manual_seed(len(name) + 17 * H)
    keep = (torch.rand((S, P.S_rows * K), generator=g) >= p_node).to(torch.uint8) if training else None
    B = P.S_rows if batch is None else batch.numel()
    G = torch.randn((S, B, H), generator=g)
    kw = dict(samples=S, dropnode_rate=p_node, input_droprate=p_in, training=training, seed=SEED)
    return {"P": P, "batch": batch, "kw": kw, "keep": keep, "G": G, "S": S, "roundings": roundings,
            "ref": ref64(P, batch, S, p_node, p_in, training, keep, SEED, G)}


def bound(terms, roundings):
    """The tolerance per element: §7d's rule up to 160 roundings, §7i's derived form beyond."""
    factor = 1e-5 if roundings <= ROUNDINGS else roundings * 2.0 ** -24
    return factor * terms.double() + 1e-7


def close(got, ref, terms, roundings, what=""):
    """Asserts |got - ref| <= bound; returns the worst error-to-bound ratio."""
    err = (got.double().cpu() - ref).abs()
    ratio = float((err / bound(terms, roundings)).max()) if err.numel() else 0.0
    assert ratio <= 1.0, f"{what}: worst error / bound {ratio:.3g}, max |d| {float(err.max()):.3e}"
    return ratio


# ---- the valid_mag / predict_mag world: sizes, the model pair and the float64 all-node embedding
MAG_V, MAG_H, MAG_C, MAG_K = 300, 64, 7, 32
EMB_SCALE, LAST_SCALE = 6.0, 4.0


def mag_attributes(n, seed=21):
    """A node-attribute CSR for n nodes: 1 .. 11 attributes each, weights in [0.05, 1.05)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 12, n)
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=indptr[1:])
    indices = rng.integers(0, MAG_V, int(indptr[-1])).astype(np.int32)
    data = (rng.random(int(indptr[-1]), dtype=np.float32) + 0.05).astype(np.float32)
    return torch.from_numpy(indptr), torch.from_numpy(indices), torch.from_numpy(data)


def mag_model_pair(seed=31):
    """(MagMLP on the CPU, oracle.mlp_ref.RefMagMLP in float64 and eval mode): equal parameters, non-trivial BatchNorm
    state; the table and the last layer are scaled so that the predictions spread and the float64 top-2 gaps are far above
    the fp32 bound for all but a few rows (asserted on the CPU in tests/test_host_mag_rows.py)."""
    from grand_plus_amd.mlp import MagMLP
    from oracle.mlp_ref import RefMagMLP
    torch.manual_seed(seed)
    ours = MagMLP(MAG_V, MAG_C, MAG_H, 2, True, 0.0, 0.5, True)
    g = torch.Generator().manual_seed(seed + 1)
    for b in ours.bns:
        b.weight.data = torch.rand(b.weight.shape, generator=g) + 0.5
        b.bias.data = torch.randn(b.bias.shape, generator=g) * 0.01
        b.running_mean.data = torch.randn(b.running_mean.shape, generator=g) * 0.01
        b.running_var.data = torch.rand(b.running_var.shape, generator=g) + 0.5
    ours.embeds.weight.data *= EMB_SCALE
    ours.fcs[-1].weight.data *= LAST_SCALE
    ref = RefMagMLP(MAG_V, MAG_C, MAG_H, 2, True, 0.0, 0.5, True)
    ref.load_state_dict(ours.state_dict())
    return ours, ref.double().eval()


def embed64(W, indptr, indices, data):
    """MLP.emb of every node in float64 (model_mag.py:48-55, eval mode): [N, H]."""
    n = indptr.numel() - 1
    node = torch.repeat_interleave(torch.arange(n), indptr[1:] - indptr[:-1])
    num = torch.zeros((n, W.shape[1]), dtype=torch.float64).index_add_(0, node, W.double()[indices.long()] * data.double()[:, None])
    den = torch.zeros((n, 1), dtype=torch.float64).index_add_(0, node, data.double()[:, None])
    return num / (den + 1e-10)


def valid_world(n=2000, n_seeds=300, n_val=200, seed=41):
    """Synthetic resident rows (every row has at least one slot), attributes, labels and an unsorted idx_val, on the CPU."""
    rng = np.random.default_rng(seed)
    seeds = np.sort(rng.choice(n, n_seeds, replace=False)).astype(np.int64)
    col = torch.from_numpy(rng.integers(0, n, (n_seeds, MAG_K)).astype(np.int32))
    val = torch.from_numpy(np.sort(rng.random((n_seeds, MAG_K)) ** 4 + 1e-9, axis=1)[:, ::-1].copy())
    filled = torch.from_numpy(rng.integers(1, MAG_K + 1, n_seeds).astype(np.int32))
    labels = torch.from_numpy(rng.integers(0, MAG_C, n))
    idx_val = torch.from_numpy(rng.permutation(seeds)[:n_val].copy())
    return {"n": n, "seeds": seeds, "col": col, "val": val, "filled": filled, "attrs": mag_attributes(n), "y": labels,
            "idx_val": idx_val}


@functools.lru_cache(maxsize=None)
def valid_reference():
    """(world, MagMLP on the CPU, the float64 chain's results on idx_val = evaluate_cases.valid64 fed the float64 all-node
    embedding), computed once."""
    import evaluate_cases as ec
    w = valid_world()
    ours, ref = mag_model_pair()
    emb = embed64(ours.embeds.weight.detach(), *w["attrs"])
    pos = torch.from_numpy(np.searchsorted(w["seeds"], w["idx_val"].numpy()))
    return w, ours, ec.valid64(ref, emb, w["col"], w["val"], w["filled"], MAG_K, pos, w["y"][w["idx_val"]])
