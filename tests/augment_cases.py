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
