"""Backward of the fused random_prop against the autograd gradient of the plain-PyTorch restatement
(oracle/random_prop_ref.py) in float64 under the same keep mask.  Tolerance per element:
|d| <= 1e-5 * sum|terms| + 1e-7, sum|terms| = the same gradient with every operand replaced by its magnitude."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu


def _close(got, ref, terms):
    import torch
    got, ref, terms = got.double().cpu(), ref.double().cpu(), terms.double().cpu()
    bad = (got - ref).abs() > 1e-5 * terms + 1e-7
    assert not bool(bad.any()), f"{int(bad.sum())} elements off; max |d| {float((got - ref).abs().max()):.3e}"


def _ragged_coo(F, seed, n_out=60, long_row=True):
    """Sorted segment ids with empty output rows in the middle and (optionally) one segment longer than the
    kernels' 1 024-entry LDS stage."""
    import torch
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(0, 40, (n_out,), generator=g)
    lens[3] = 0; lens[4] = 0; lens[17] = 0; lens[-1] = 5
    if long_row:
        lens[10] = 1100
    idx = torch.repeat_interleave(torch.arange(n_out), lens)
    M = idx.numel()
    feats = torch.randn((M, F), generator=g, dtype=torch.float64)
    scores = (torch.rand((M,), generator=g, dtype=torch.float64) ** 2 + 1e-6).float()
    return feats, scores, idx, g


def _ref_grad(feats64, scores, idx, p, training, keep, G64):
    from oracle.random_prop_ref import random_prop_ref
    x = feats64.clone().requires_grad_(True)
    out = random_prop_ref(x, scores.double(), idx, p, training, keep)
    (out * G64).sum().backward()
    xa = feats64.abs().clone().requires_grad_(True)
    outa = random_prop_ref(xa, scores.double().abs(), idx, p, training, keep)
    (outa * G64.abs()).sum().backward()
    return out.detach(), x.grad, xa.grad


@pytest.mark.parametrize("F", [7, 64, 602])
@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.5, 1.0])
def test_coo_backward_matches_reference_gradient(F, training, p):
    import torch
    from grand_plus_amd.augment import random_prop
    feats64, scores, idx, g = _ragged_coo(F, seed=F * 7 + int(p * 10) + training)
    keep = (torch.rand(scores.shape, generator=g) >= p).to(torch.uint8)
    n_out = int(idx[-1]) + 1
    G = torch.randn((n_out, F), generator=g, dtype=torch.float32)
    ref_out, ref_grad, terms = _ref_grad(feats64, scores, idx, p, training, keep, G.double())
    x = feats64.float().cuda().requires_grad_(True)
    out = random_prop(x, scores.cuda(), idx.cuda(), p, training=training, keep=keep.cuda())
    assert out.grad_fn is not None
    out.backward(G.cuda())
    assert x.grad.shape == (idx.numel(), F)
    _close(x.grad, ref_grad, terms)
    if training and p == 1.0:
        assert torch.count_nonzero(x.grad) == 0
    # dropped entries get exact zeros
    if training:
        assert torch.count_nonzero(x.grad.cpu()[keep == 0]) == 0


def _rows_case(seed=0, S=120, K=32, N=3000, F=64):
    import torch
    g = torch.Generator().manual_seed(seed)
    col = torch.randint(0, N, (S, K), generator=g, dtype=torch.int32)
    col[:, 0] = 7                                   # node 7 in every row ...
    col[5, 9] = 7                                   # ... and twice in row 5
    col[11, 3] = col[11, 20] = 42                   # another node twice in one row
    val = torch.rand((S, K), generator=g, dtype=torch.float64) ** 3 + 1e-9
    filled = torch.randint(1, K + 1, (S,), generator=g, dtype=torch.int32)
    filled[5] = K; filled[11] = K
    X = torch.randn((N, F), generator=g, dtype=torch.float32)
    return col, val, filled, X, g


@pytest.mark.parametrize("F", [7, 64, 602])
@pytest.mark.parametrize("training", [False, True])
def test_rows_backward_matches_reference_gradient(F, training):
    import torch
    from grand_plus_amd.augment import random_prop_rows
    from oracle.random_prop_ref import random_prop_ref
    col, val, filled, X, g = _rows_case(seed=F, F=F)
    S, K = col.shape
    rows = torch.randperm(S, generator=g)[:90].to(torch.int32)
    rows[:2] = torch.tensor([5, 11], dtype=torch.int32)
    p = 0.5
    keep_rows = (torch.rand((S, K), generator=g) >= p).to(torch.uint8)
    keep_rows[5, 0] = keep_rows[5, 9] = 1
    # the flattened (reference) form of the same batch and mask
    idx, cols, sc, kp = [], [], [], []
    for b, r in enumerate(rows.tolist()):
        n = int(filled[r])
        idx += [b] * n; cols += col[r, :n].tolist(); sc += val[r, :n].tolist(); kp += keep_rows[r, :n].tolist()
    idx = torch.tensor(idx); cols = torch.tensor(cols, dtype=torch.int64)
    scores = torch.tensor(sc, dtype=torch.float64).float(); kp = torch.tensor(kp, dtype=torch.uint8)
    G = torch.randn((rows.numel(), F), generator=g)
    X64 = X.double().requires_grad_(True)
    (random_prop_ref(X64[cols], scores.double(), idx, p, training, kp) * G.double()).sum().backward()
    Xa = X.double().abs().requires_grad_(True)
    (random_prop_ref(Xa[cols], scores.double(), idx, p, training, kp) * G.double().abs()).sum().backward()
    x = X.cuda().requires_grad_(True)
    out = random_prop_rows(x, col.reshape(-1).cuda(), val.reshape(-1).cuda(), filled.cuda(), K, batch_rows=rows.cuda(),
                           dropnode_rate=p, training=training, keep=keep_rows.reshape(-1).cuda())
    out.backward(G.cuda())
    _close(x.grad, X64.grad, Xa.grad)
    assert float(x.grad[7].abs().sum()) > 0


def test_internal_rng_mask_is_the_forwards_mask():
    """Zero rows of grad_feats are the dropped entries: the forward with that mask as an explicit `keep` equals
    the internal-RNG forward bitwise.  The same for the fused form, whose rows here hold distinct nodes."""
    import torch
    from grand_plus_amd.augment import random_prop, random_prop_rows
    feats64, scores, idx, g = _ragged_coo(64, seed=3)
    x = feats64.float().cuda().requires_grad_(True)
    sc, ic = scores.cuda(), idx.cuda()
    out = random_prop(x, sc, ic, 0.5, training=True, seed=1234)
    out.backward(torch.ones_like(out))
    keep = (x.grad.abs().sum(1) != 0).to(torch.uint8)
    assert 0.4 < float(keep.float().mean()) < 0.6
    with torch.no_grad():
        explicit = random_prop(x, sc, ic, 0.5, training=True, keep=keep)
    assert torch.equal(explicit, out.detach())
    # fused form: every slot of the batch a different node, so grad_X[node] != 0 iff that slot was kept
    S, K, N, F = 50, 16, 2000, 32
    col = torch.randperm(N, generator=g)[:S * K].to(torch.int32)
    val = torch.rand(S * K, generator=g, dtype=torch.float64) + 0.1
    filled = torch.full((S,), K, dtype=torch.int32)
    X = torch.randn((N, F), generator=g).cuda().requires_grad_(True)
    rows = torch.arange(S, dtype=torch.int32).cuda()
    out = random_prop_rows(X, col.cuda(), val.cuda(), filled.cuda(), K, batch_rows=rows, dropnode_rate=0.5, training=True, seed=77)
    out.backward(torch.ones_like(out))
    keep_rows = (X.grad.abs().sum(1)[col.long().cuda()] != 0).to(torch.uint8)
    with torch.no_grad():
        explicit = random_prop_rows(X, col.cuda(), val.cuda(), filled.cuda(), K, batch_rows=rows, dropnode_rate=0.5, training=True,
                                    keep=keep_rows)
    assert torch.equal(explicit, out.detach())


def test_nothing_changes_without_grad():
    import torch
    from grand_plus_amd import _native
    from grand_plus_amd.augment import random_prop, random_prop_rows
    feats64, scores, idx, g = _ragged_coo(96, seed=5, long_row=False)
    f, sc, ic = feats64.float().cuda(), scores.cuda(), idx.cuda()
    n_out = int(idx[-1]) + 1
    direct = torch.empty((n_out, 96), device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    _native.raise_for_status(_native.lib().gp_random_prop_coo(
        0, f.data_ptr(), f.shape[0], 96, sc.data_ptr(), ic.data_ptr(), n_out, 0.5, 1, ctypes.c_uint64(99), None,
        direct.data_ptr(), ctypes.c_void_p(stream)))
    a = random_prop(f, sc, ic, 0.5, training=True, seed=99)                          # input does not require grad
    fr = f.clone().requires_grad_(True)
    with torch.no_grad():
        b = random_prop(fr, sc, ic, 0.5, training=True, seed=99)                     # grad disabled
    c = random_prop(fr, sc, ic, 0.5, training=True, seed=99)                         # the autograd path
    assert a.grad_fn is None and b.grad_fn is None and not a.requires_grad and not b.requires_grad
    assert torch.equal(a, direct) and torch.equal(b, direct) and torch.equal(c.detach(), direct)
    assert c.grad_fn is not None
    # fused form
    col, val, filled, X, g = _rows_case(seed=9)
    S, K = col.shape
    Xc, cc, vc, fc = X.cuda(), col.reshape(-1).cuda(), val.reshape(-1).cuda(), filled.cuda()
    rows = torch.arange(0, S, 3, dtype=torch.int32).cuda()
    direct = torch.empty((rows.numel(), X.shape[1]), device="cuda")
    _native.raise_for_status(_native.lib().gp_random_prop_rows(
        0, Xc.data_ptr(), X.shape[0], X.shape[1], cc.data_ptr(), vc.data_ptr(), fc.data_ptr(), K, rows.data_ptr(), rows.numel(),
        0.5, 1, ctypes.c_uint64(5), None, direct.data_ptr(), ctypes.c_void_p(stream)))
    a = random_prop_rows(Xc, cc, vc, fc, K, batch_rows=rows, dropnode_rate=0.5, training=True, seed=5)
    Xr = Xc.clone().requires_grad_(True)
    with torch.no_grad():
        b = random_prop_rows(Xr, cc, vc, fc, K, batch_rows=rows, dropnode_rate=0.5, training=True, seed=5)
    c = random_prop_rows(Xr, cc, vc, fc, K, batch_rows=rows, dropnode_rate=0.5, training=True, seed=5)
    assert a.grad_fn is None and b.grad_fn is None
    assert torch.equal(a, direct) and torch.equal(b, direct) and torch.equal(c.detach(), direct)
    assert c.grad_fn is not None
