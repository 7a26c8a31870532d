"""Inputs, the reference's COO form of a batch of rows, reference gradients and the tolerance shared by the random_prop
and embedding tests.  The reference itself is oracle/random_prop_ref.py."""
import torch

from oracle.random_prop_ref import random_prop_ref


def close(got, ref, terms):
    """§7d's tolerance per element: |d| <= 1e-5 * sum|terms| + 1e-7, sum|terms| = the reference quantity with every
    operand replaced by its magnitude."""
    got, ref, terms = got.double().cpu(), ref.double().cpu(), terms.double().cpu()
    bad = (got - ref).abs() > 1e-5 * terms + 1e-7
    assert not bool(bad.any()), f"{int(bad.sum())} elements off; max |d| {float((got - ref).abs().max()):.3e}"


def ragged_coo(F, seed, n_out, dtype=torch.float32, long_row=True):
    """(feats [M, F] in dtype, scores float32, idx, generator): sorted segment ids with empty output rows in the middle
    and (optionally) one segment longer than the kernels' 1 024-entry LDS stage.  Features and scores are drawn in dtype."""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(0, 40, (n_out,), generator=g)
    lens[3] = 0; lens[4] = 0; lens[17] = 0; lens[-1] = 5
    if long_row:
        lens[10] = 1100
    idx = torch.repeat_interleave(torch.arange(n_out), lens)
    M = idx.numel()
    feats = torch.randn((M, F), generator=g, dtype=dtype)
    scores = (torch.rand((M,), generator=g, dtype=dtype) ** 2 + 1e-6).float()
    return feats, scores, idx, g


def rows_case(seed=0, S_rows=120, K=32, N=3000, F=64, empty_row=None, second_duplicate=False):
    """(col [S_rows, K], val, filled, X [N, F], generator): resident rows with node 7 in every row and twice in the full
    row 5; optionally an empty row, and a second node twice in the full row 11."""
    g = torch.Generator().manual_seed(seed)
    col = torch.randint(0, N, (S_rows, K), generator=g, dtype=torch.int32)
    col[:, 0] = 7
    col[5, 9] = 7
    if second_duplicate:
        col[11, 3] = col[11, 20] = 42
    val = torch.rand((S_rows, K), generator=g, dtype=torch.float64) ** 3 + 1e-9
    filled = torch.randint(1, K + 1, (S_rows,), generator=g, dtype=torch.int32)
    filled[5] = K
    if second_duplicate:
        filled[11] = K
    if empty_row is not None:
        filled[empty_row] = 0
    X = torch.randn((N, F), generator=g, dtype=torch.float32)
    return col, val, filled, X, g


def rows_to_coo(col, val, filled, K, rows, keep=None):
    """What the reference's caller builds on the host for a batch (model.py:310-316): the filled slots of the resident
    [S_rows x K] rows `rows`, one after another.  Returns (idx, cols, scores, kp): the output row of each entry, its
    node id (int64), its score (float32, model.py:314) and, for keep = S masks over the S_rows * K slots (any shape
    [S, ...]), the same masks over the entries, [S, M]; None without keep."""
    col, val, r = col.reshape(-1, K), val.reshape(-1, K), rows.long()
    n = filled.long()[r]
    sel = torch.arange(K)[None, :] < n[:, None]
    idx = torch.repeat_interleave(torch.arange(r.numel()), n)
    kp = None if keep is None else keep.reshape(-1, col.shape[0], K)[:, r][:, sel]
    return idx, col[r][sel].long(), val[r][sel].float(), kp


def ref_grad(x, scores, idx, p, training, keep, G, cols=None):
    """Float64 autograd gradient with respect to x of sum_s <random_prop_ref(feats, mask s), G[s]>, feats = x (COO form)
    or x[cols] (rows form), for one mask (keep [M], G [n_out, F]) or S masks (keep [S, M], G [S, n_out, F]); and the
    same with every operand replaced by its magnitude, which `close` takes as `terms`."""
    if G.dim() == 2:
        keep, G = keep[None], G[None]
    n_out = int(idx[-1]) + 1
    scores = scores.double()
    x64 = x.detach().double().clone().requires_grad_(True)
    xa = x.detach().double().abs().requires_grad_(True)
    for k, g in zip(keep, G.double()[:, :n_out]):
        for leaf, sc, gg in ((x64, scores, g), (xa, scores.abs(), g.abs())):
            feats = leaf if cols is None else leaf[cols]
            (random_prop_ref(feats, sc, idx, p, training, k) * gg).sum().backward()
    return x64.grad, xa.grad


def emb_ref(W, attr_idx, node_idx, attr_data, p, training, keep):
    """MLP.emb (model_mag.py:48-55) in the dtype of W; keep: [nnz, H] 0/1 mask of F.dropout."""
    fe = W[attr_idx]                                                             # self.embeds(attr_idx)
    if training:                                                                 # F.dropout(feat_embeds, p)
        fe = fe * keep.to(fe.dtype) / (1.0 - p) if p < 1.0 else torch.zeros_like(fe)
    d = attr_data.to(fe.dtype)
    n_out = int(node_idx[-1]) + 1
    num = torch.zeros((n_out, W.shape[1]), dtype=fe.dtype).index_add_(0, node_idx, fe * d[:, None])
    den = torch.zeros((n_out, 1), dtype=fe.dtype).index_add_(0, node_idx, d[:, None])
    return num / (den + 1e-10)


# ---- The edge cases of csrc/augment.hip ("Pinned edges of random_prop and the embedding bag"): shared by
# tests/test_gpu_augment_edges.py (the kernels against float64) and tests/test_host_augment_edges.py (the cases themselves:
# a float32 restatement in the kernels' order stays inside the tolerance, and every sentinel is visible to it).

A_K = (1, 7, 8, 9, 255, 256, 257, 1023, 1024)                  # group A: staging trips and the 8-wide unroll
B_K, B_S, B_COO_S = (32, 963, 1024), (4, 5, 7, 8, 9, 15, 16), (5, 8, 9, 16)   # group B: sample chunks
C_F = (1, 2, 3, 4, 6, 1024, 1028, 1030, 1433)                  # group C: VEC, feature slabs, a slab with one live lane
D_ROWS = 65535 + 41                                            # group D: the second trip of the grid-stride loops
E_LENS = (0, 0, 1023, 1024, 1025, 0, 3, 1, 9, 8)               # group E: segments round the 1 024-entry stage
G_H = (1, 2, 3, 4, 5, 6, 8, 12, 16, 17, 33, 63, 65, 128, 129, 130, 256, 257, 260, 516)   # group G: log2g 0-6, every VEC, n_f <= 9
G_LENS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 0, 200)
G_CSR_H = (3, 12, 129, 260)
N_SENT = 32                                                    # ids [0, N_SENT) are kept for the sentinels
P_DROP = 0.5


class Case:
    """Plain attribute bag of one case's tensors (all on the CPU)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def sentinel_slots(n):
    """The slots of an n-entry row at which the random_prop kernels change trips: the first and last, the last of the
    8-wide unrolled loop and the first of its tail, and both sides of every 256-entry staging pass."""
    marks = {0, 8 * (n // 8) - 1, 8 * (n // 8), 255, 256, 511, 512, 767, 768, n - 1}
    return sorted(k for k in marks if 0 <= k < n)


def bag_sentinel_slots(n):
    """The same for a bag: entry 0, G - 1 and G for every lane group G = 1 .. 64, 63 | 64 of the backward's read round, last."""
    marks = {0, 1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64, n - 1}
    return sorted(k for k in marks if 0 <= k < n)


def _loud(x):
    """x with every magnitude raised to >= 1, signs kept."""
    return torch.where(x < 0, -1.0, 1.0).to(x.dtype) * (1 + x.abs())


def edge_rows(K, F, S, seed, N=300, filled=None, rows=None):
    """A rows-form case: resident rows [R, K] with `filled` (default: K, 1, 0, 8*(K//8), K - 1 and K + 5, which the
    kernels clamp to K), a batch of B = 8 rows that names the full row and the empty row twice, S explicit masks at
    p = 0.5 and upstream gradients G [S, B, F].  Sentinels: at sentinel_slots(n) of every row the weight is 1.0 (every
    other weight lies in [0.01, 0.25]) on a node of its own among ids [0, N_SENT), whose features have magnitude >= 1,
    and the slot is kept in at least one sample.  Slots past `filled` hold a valid node and the weight 5: a kernel that
    read one would show."""
    g = torch.Generator().manual_seed(seed)
    filled = torch.tensor([K, 1, 0, 8 * (K // 8), K - 1, K + 5] if filled is None else filled, dtype=torch.int32)
    R = filled.numel()
    rows = torch.tensor([3, 0, 1, 2, 0, 4, 5, 2] if rows is None else rows, dtype=torch.int32)
    col = torch.randint(N_SENT, N, (R, K), generator=g, dtype=torch.int32)
    val = torch.rand((R, K), generator=g, dtype=torch.float64) * 0.24 + 0.01
    X = torch.randn((N, F), generator=g)
    X[:N_SENT] = _loud(X[:N_SENT])
    keep = (torch.rand((S, R, K), generator=g) >= P_DROP).to(torch.uint8)
    sent = torch.zeros((R, K), dtype=torch.bool)
    for r in range(R):
        n = min(int(filled[r]), K)
        val[r, n:] = 5.0
        for i, k in enumerate(sentinel_slots(n)):
            col[r, k], val[r, k], keep[(r + i) % S, r, k], sent[r, k] = i, 1.0, 1, True
    G = torch.randn((S, rows.numel(), F), generator=g)
    return Case(K=K, F=F, S=S, N=N, col=col, val=val, filled=filled, rows=rows, X=X, keep=keep, G=G, sent=sent, p=P_DROP)


def second_trip_rows(S, seed=77):
    """Group D: 65 535 + 41 batch rows drawn from 50 resident rows of K = 2 with 0, 1 or 2 filled slots, F = 4, N = 20 000.
    Every slot has a node of its own (every filled slot of so short a row is a sentinel), so the fused backward spreads
    its atomic adds over as many destination rows as 50 resident rows can name."""
    g = torch.Generator().manual_seed(seed)
    filled = torch.randint(0, 3, (50,), generator=g).tolist()
    filled[:3] = [2, 1, 0]
    rows = torch.randint(0, 50, (D_ROWS,), generator=g).tolist()
    rows[-3:] = [0, 2, 1]
    c = edge_rows(2, 4, S, seed, N=20000, filled=filled, rows=rows)
    c.col = (N_SENT + 199 * torch.arange(100, dtype=torch.int32)).reshape(50, 2)
    c.X[c.col.long().reshape(-1)] = _loud(c.X[c.col.long().reshape(-1)])
    return c


def score_rows(S, seed=5):
    """Group F (K = 9, F = 12, every row full): row 1 has 1e-60 (0 in float32) in every other slot, row 2 in every slot,
    row 3 holds 1e-13 throughout, so that its denominator is of the size of the 1e-12 epsilon."""
    c = edge_rows(9, 12, S, seed, filled=[9] * 6)
    c.val[1, 1::2] = 1e-60
    c.val[2, :] = 1e-60
    c.val[3, :] = 1e-13
    c.sent &= c.val == 1.0
    return c


def coo_view(c, keep=None):
    """The COO form of a rows case (what the reference's caller gathers, model.py:310-316): a Case with feats = X[cols],
    scores (float32), idx, cols, n_out = B, keep [S, M], and the sentinel flag of every entry."""
    fl = c.filled.clamp(max=c.K)
    idx, cols, scores, kp = rows_to_coo(c.col, c.val, fl, c.K, c.rows, c.keep if keep is None else keep)
    sent = rows_to_coo(c.col, c.val, fl, c.K, c.rows, c.sent[None].to(torch.uint8))[3][0].bool()
    return Case(F=c.F, S=c.S, feats=c.X[cols], scores=scores, idx=idx, cols=cols, n_out=c.rows.numel(), keep=kp, G=c.G,
                sent=sent, p=c.p, N=c.N)


def edge_coo(F, S, seed, lens=E_LENS):
    """A COO case: sorted segment ids with segments of `lens` entries (group E: two leading empty rows, then 1 023, 1 024
    and 1 025 entries: the last staged lengths and the first on the plain loop), sentinels as edge_rows'."""
    g = torch.Generator().manual_seed(seed)
    lens = torch.tensor(lens)
    idx = torch.repeat_interleave(torch.arange(lens.numel()), lens)
    M = idx.numel()
    feats = torch.randn((M, F), generator=g)
    scores = (torch.rand((M,), generator=g) * 0.24 + 0.01).float()
    keep = (torch.rand((S, M), generator=g) >= P_DROP).to(torch.uint8)
    sent = torch.zeros(M, dtype=torch.bool)
    start = torch.cumsum(lens, 0) - lens
    for b in range(lens.numel()):
        for i, k in enumerate(sentinel_slots(int(lens[b]))):
            e = int(start[b]) + k
            scores[e], keep[(b + i) % S, e], sent[e] = 1.0, 1, True
    feats[sent] = _loud(feats[sent])
    n_out = int(idx[-1]) + 1
    G = torch.randn((S, n_out, F), generator=g)
    return Case(F=F, S=S, feats=feats, scores=scores, idx=idx, cols=None, n_out=n_out, keep=keep, G=G, sent=sent, p=P_DROP)


def coo_reference(c, training, n_out=None):
    """(ref, terms) [S, n_out, F]: oracle.random_prop_ref in float64 per sample under the case's masks, rows past the
    last segment zero; terms = the same with every operand replaced by its magnitude."""
    n_out = c.n_out if n_out is None else n_out
    ref = torch.zeros((c.S, n_out, c.F), dtype=torch.float64)
    terms = torch.zeros_like(ref)
    if c.idx.numel():
        f, sc = c.feats.double(), c.scores.double()
        for s in range(c.S):
            r = random_prop_ref(f, sc, c.idx, c.p, training, c.keep[s])
            ref[s, :r.shape[0]] = r
            terms[s, :r.shape[0]] = random_prop_ref(f.abs(), sc.abs(), c.idx, c.p, training, c.keep[s])
    return ref, terms


def coo_ref_grad(c, training, x=None):
    """ref_grad of a COO case or view: with respect to the feats, or to x = the rows case's X through the view's cols."""
    return ref_grad(c.feats if x is None else x, c.scores, c.idx, c.p, training, c.keep, c.G, cols=None if x is None else c.cols)


def bound(terms):
    """The tolerance of `close` as a tensor."""
    return 1e-5 * terms.double() + 1e-7


def f32_random_prop(c, training):
    """numpy float32 restatement of the random_prop kernels on a COO case, in their order: per sample den left to right
    over the row's entries, inv = 1 / (den + 1e-12f), each column's sum left to right with the product rounded before
    the add, then * inv.  Returns (out [S, n_out, F], inv [S, n_out], w [S, M])."""
    import numpy as np
    f4 = np.float32
    feats, scores, idx = c.feats.numpy().astype(f4), c.scores.numpy().astype(f4), c.idx.numpy()
    lens = np.bincount(idx, minlength=c.n_out)
    start = np.cumsum(lens) - lens
    scale = f4(1.0) / (f4(1.0) - f4(c.p))
    out = np.zeros((c.S, c.n_out, c.F), f4)
    inv = np.zeros((c.S, c.n_out), f4)
    ws = np.zeros((c.S, idx.size), f4)
    for s in range(c.S):
        w = scores * np.where(c.keep[s].numpy() != 0, scale, f4(0.0)).astype(f4) if training else scores
        den, acc = np.zeros(c.n_out, f4), np.zeros((c.n_out, c.F), f4)
        for k in range(int(lens.max()) if lens.size else 0):
            live = lens > k
            e = start[live] + k
            den[live] += w[e]
            acc[live] += w[e][:, None] * feats[e]
        inv[s] = f4(1.0) / (den + f4(1e-12))
        out[s] = acc * inv[s][:, None]
        ws[s] = w
    return out, inv, ws


def f32_random_prop_grad(c, training, n_nodes=None):
    """The backward in float32: per entry (g * inv) * w summed over s in order; with n_nodes the entries are then added
    into X's gradient [n_nodes, F] one after another (the fused form), else returned as the COO gradient [M, F]."""
    import numpy as np
    _, inv, ws = f32_random_prop(c, training)
    idx, G = c.idx.numpy(), c.G.numpy().astype(np.float32)
    ge = np.zeros((idx.size, c.F), np.float32)
    for s in range(c.S):
        ge += (G[s][idx] * inv[s][idx][:, None]) * ws[s][:, None]
    if n_nodes is None:
        return ge
    gx = np.zeros((n_nodes, c.F), np.float32)
    np.add.at(gx, c.cols.numpy(), ge)
    return gx


def sentinel_margin(c, training):
    """The smallest, over the case's sentinel entries, of the largest ratio |shift| / bound that taking the entry out of
    the float64 reference (its score set to 0 in a sample that keeps it) causes in any element of the output."""
    f, sc = c.feats.double(), c.scores.double()
    eps, worst = 1e-12, float("inf")
    best = torch.zeros(c.idx.numel(), dtype=torch.float64)
    for s in range(c.S):
        w = sc * (c.keep[s].double() / (1.0 - c.p)) if training else sc
        num = torch.zeros((c.n_out, c.F), dtype=torch.float64).index_add_(0, c.idx, f * w[:, None])
        absn = torch.zeros((c.n_out, c.F), dtype=torch.float64).index_add_(0, c.idx, f.abs() * w[:, None])
        den = torch.zeros((c.n_out,), dtype=torch.float64).index_add_(0, c.idx, w)
        nb, db, ab = num[c.idx], den[c.idx][:, None], absn[c.idx]
        shift = ((nb - f * w[:, None]) / (db - w[:, None] + eps) - nb / (db + eps)).abs()
        best = torch.maximum(best, (shift / bound(ab / (db + eps))).max(1).values)
    if bool(c.sent.any()):
        worst = float(best[c.sent].min())
    return worst


def ratio(got, ref, terms):
    """Largest |got - ref| / bound(terms)."""
    got = torch.as_tensor(got).double()
    return float(((got - ref.double()).abs() / bound(terms)).max()) if got.numel() else 0.0


def edge_bags(H, seed, V=300):
    """Group G: one bag of each length in G_LENS (the first and one more empty), ids drawn from [N_SENT, 250) so that they
    repeat within and across bags and rows 250 .. V - 1 of the table are named by no bag, every seventh weight zero, an
    explicit element mask at p = 0.5.  Sentinels: at bag_sentinel_slots(len) the weight is 1.0 (every other in [0.01, 0.25])
    on an id of its own among [0, N_SENT), whose table row has magnitude >= 1, and every element of the entry is kept."""
    g = torch.Generator().manual_seed(seed)
    lens = torch.tensor(G_LENS)
    node_idx = torch.repeat_interleave(torch.arange(lens.numel()), lens)
    nnz = node_idx.numel()
    attr_idx = torch.randint(N_SENT, 250, (nnz,), generator=g)
    attr_data = torch.rand((nnz,), generator=g) * 0.24 + 0.01
    attr_data[::7] = 0.0
    keep = (torch.rand((nnz, H), generator=g) >= P_DROP).to(torch.uint8)
    W = torch.randn((V, H), generator=g)
    W[:N_SENT] = _loud(W[:N_SENT])
    sent = torch.zeros(nnz, dtype=torch.bool)
    start = torch.cumsum(lens, 0) - lens
    for b in range(lens.numel()):
        if int(lens[b]) > 40:
            attr_idx[int(start[b]) + 21] = attr_idx[int(start[b]) + 20]            # an id twice inside one bag
        for i, k in enumerate(bag_sentinel_slots(int(lens[b]))):
            e = int(start[b]) + k
            attr_idx[e], attr_data[e], keep[e], sent[e] = i, 1.0, 1, True
    G = torch.randn((int(node_idx[-1]) + 1, H), generator=g)
    return Case(H=H, V=V, W=W, attr_idx=attr_idx, node_idx=node_idx, attr_data=attr_data, keep=keep, G=G, sent=sent,
                lens=lens, p=P_DROP, n_out=int(node_idx[-1]) + 1)


def bag_reference(c, training):
    """(out, terms, dW, dW terms) of emb_ref in float64 through autograd under the case's mask and G."""
    w = c.W.double().requires_grad_(True)
    wa = c.W.double().abs().requires_grad_(True)
    ref = emb_ref(w, c.attr_idx, c.node_idx, c.attr_data, c.p, training, c.keep)
    (ref * c.G.double()).sum().backward()
    terms = emb_ref(wa, c.attr_idx, c.node_idx, c.attr_data, c.p, training, c.keep)
    (terms * c.G.double().abs()).sum().backward()
    return ref.detach(), terms.detach(), w.grad, wa.grad


def f32_bag(c, training):
    """numpy float32 restatement of the bag kernels: (out, dW).  Forward: x = W[a] * keep-scale, acc += x * d entry after
    entry, den += d likewise, out = acc / (den + 1e-10f).  Backward: ((g * inv) * d) * keep-scale added row after row."""
    import numpy as np
    f4 = np.float32
    W, a, m, d = c.W.numpy().astype(f4), c.attr_idx.numpy(), c.node_idx.numpy(), c.attr_data.numpy().astype(f4)
    scale = f4(1.0) / (f4(1.0) - f4(c.p))
    ks = np.where(c.keep.numpy() != 0, scale, f4(0.0)).astype(f4) if training else np.ones((a.size, c.H), f4)
    lens = np.bincount(m, minlength=c.n_out)
    start = np.cumsum(lens) - lens
    den, acc = np.zeros(c.n_out, f4), np.zeros((c.n_out, c.H), f4)
    for k in range(int(lens.max())):
        live = lens > k
        e = start[live] + k
        den[live] += d[e]
        acc[live] += (W[a[e]] * ks[e]) * d[e][:, None]
    out = acc / (den + f4(1e-10))[:, None]
    inv = f4(1.0) / (den + f4(1e-10))
    dW = np.zeros_like(W)
    np.add.at(dW, a, ((c.G.numpy().astype(f4)[m] * inv[m][:, None]) * d[:, None]) * ks)
    return out, dW


def bag_sentinel_margin(c, training):
    """sentinel_margin for a bag case: the entry's weight set to 0 (numerator and denominator)."""
    w = c.W.double()[c.attr_idx] * (c.keep.double() / (1.0 - c.p) if training else 1.0)
    d = c.attr_data.double()[:, None]
    z = torch.zeros((c.n_out, c.H), dtype=torch.float64)
    num, absn = z.clone().index_add_(0, c.node_idx, w * d), z.clone().index_add_(0, c.node_idx, w.abs() * d)
    den = torch.zeros((c.n_out, 1), dtype=torch.float64).index_add_(0, c.node_idx, d)
    nb, db, ab = num[c.node_idx], den[c.node_idx], absn[c.node_idx]
    shift = ((nb - w * d) / (db - d + 1e-10) - nb / (db + 1e-10)).abs()
    return float((shift / bound(ab / (db + 1e-10))).max(1).values[c.sent].min())


def bags_as_csr(c):
    """The bags as a node-attribute CSR (indptr int64, indices int32, data) and `nodes` out of order with one repeat; and
    the COO form of those nodes' bags one after another (attr_idx int64, node_idx, attr_data)."""
    lens = c.lens
    indptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)])
    nodes = torch.randperm(lens.numel(), generator=torch.Generator().manual_seed(3))
    nodes = torch.cat([nodes[:9], nodes[4:5], nodes[9:]])
    pos = torch.cat([torch.arange(int(indptr[n]), int(indptr[n + 1])) for n in nodes.tolist()])
    node_idx = torch.repeat_interleave(torch.arange(nodes.numel()), lens[nodes])
    return indptr, c.attr_idx.to(torch.int32), c.attr_data, nodes, c.attr_idx[pos], node_idx, c.attr_data[pos]


# ---- the two operations written out, and one deliberate mistake (tests/test_host_mutants.py)
MUTANTS = ("den_no_eps", "den_eps_swapped", "den_max", "keep_scale_missing", "sample0_mask_for_all", "bag_not_normalised")
TINY_BAG, TINY_WEIGHT = 8, 1e-11           # edge_bags' bag of 9 entries; 9 weights of 1e-11 sum to the 1e-10 beside them
TINY_BAG_H = (12, 65)


def divide(num, den, eps, other, mut):
    """num / (den + eps), or what a mistaken denominator gives: none, the other operation's epsilon, max(den, eps)."""
    if mut == "den_no_eps":
        return num / den
    if mut == "den_eps_swapped":
        return num / (den + other)
    if mut == "den_max":
        return num / den.clamp(min=eps)
    return num / (den + eps)


def coo_manual64(c, training, mut=None):
    """coo_reference's first result from explicit formulas (mut None), or with one of MUTANTS built in."""
    out = torch.zeros((c.S, c.n_out, c.F), dtype=torch.float64)
    f, sc = c.feats.double(), c.scores.double()
    scale = 1.0 if mut == "keep_scale_missing" and c.p < 1.0 else (1.0 / (1.0 - c.p) if c.p < 1.0 else 0.0)
    for s in range(c.S if c.idx.numel() else 0):
        w = sc * c.keep[0 if mut == "sample0_mask_for_all" else s].double() * scale if training else sc
        num = torch.zeros((c.n_out, c.F), dtype=torch.float64).index_add_(0, c.idx, f * w[:, None])
        den = torch.zeros((c.n_out, 1), dtype=torch.float64).index_add_(0, c.idx, w[:, None])
        out[s] = num if mut == "bag_not_normalised" else divide(num, den, 1e-12, 1e-10, mut)
    return out


def bag_manual64(c, training, mut=None):
    """bag_reference's first result from explicit formulas (mut None), or with one of MUTANTS built in."""
    fe = c.W.double()[c.attr_idx]
    if training:
        scale = 1.0 if mut == "keep_scale_missing" and c.p < 1.0 else (1.0 / (1.0 - c.p) if c.p < 1.0 else 0.0)
        fe = fe * c.keep.double() * scale
    d = c.attr_data.double()[:, None]
    num = torch.zeros((c.n_out, c.H), dtype=torch.float64).index_add_(0, c.node_idx, fe * d)
    den = torch.zeros((c.n_out, 1), dtype=torch.float64).index_add_(0, c.node_idx, d)
    return num if mut == "bag_not_normalised" else divide(num, den, 1e-10, 1e-12, mut)


def finite_ratio(got, ref, terms):
    """(`ratio` over the elements where `got` is finite, whether some element is not)."""
    got = torch.as_tensor(got).double()
    ok = torch.isfinite(got)
    r = ((got - ref.double()).abs() / bound(terms))[ok]
    return (float(r.max()) if r.numel() else 0.0), not bool(ok.all())


def tiny_bags(H):
    """edge_bags(H) with the 9 weights of bag TINY_BAG at 1e-11: its denominator is of the size of the bag's 1e-10."""
    c = edge_bags(H, seed=H)
    assert int(c.lens[TINY_BAG]) == 9
    e = c.node_idx == TINY_BAG
    c.attr_data[e] = TINY_WEIGHT
    c.sent = c.sent & ~e
    return c


def drawn_forward():
    """The forward cases tests/test_gpu_augment_edges.py holds to float64, as (name, kind, case, training), kind "coo" (a COO
    case or the COO view of a rows case) or "bag": groups A (K up to 257), C, E, F and G with the file's own parameters and
    seeds, and the bags at the epsilon's scale."""
    for training in (False, True):
        for S in (1, 2):
            for K in (k for k in A_K if k <= 257):
                for F in (12, 65):
                    yield f"A K={K} F={F} S={S} training={training}", "coo", coo_view(edge_rows(K, F, S, seed=K + F + S)), training
            yield f"E S={S} training={training}", "coo", edge_coo(6, S, seed=40 + S), training
            yield f"F S={S} training={training}", "coo", coo_view(score_rows(S)), training
        for S in (1, 3):
            for F in C_F:
                yield f"C F={F} S={S} training={training}", "coo", coo_view(edge_rows(9, F, S, seed=F + S)), training
        for H in G_H:
            yield f"G H={H} training={training}", "bag", edge_bags(H, seed=H), training
        for H in TINY_BAG_H:
            yield f"tiny bag H={H} training={training}", "bag", tiny_bags(H), training
