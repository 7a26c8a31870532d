"""S-sample random_prop: out[s] of one S-sample launch equals the single-sample call with
sample_seed(seed, s) (or keep[s]) bit for bit, and both backwards match the float64 autograd gradient of
oracle.random_prop_ref summed over the samples under the same masks.  Tolerance per element (§7d):
|d| <= 1e-5 * sum|terms| + 1e-7, sum|terms| = the same gradient with every operand replaced by its magnitude."""
import pytest

from augment_cases import close, ragged_coo, ref_grad, rows_case, rows_to_coo

pytestmark = pytest.mark.gpu


def _coo_multi(feats, scores, idx, n_out, S, p, training, seed=None, keep=None):
    """The S-sample COO entry (S = 1 included: random_prop(samples=1) takes the single-sample entry)."""
    import torch
    from grand_plus_amd import augment
    if S > 1:
        return augment.random_prop(feats, scores, idx, p, training=training, seed=seed, keep=keep, samples=S, n_out=n_out)
    stream = torch.cuda.current_stream().cuda_stream
    return augment._coo_multi_forward(feats, scores, idx, n_out, 1, p, training, seed if seed is not None else 7,
                                      keep.reshape(-1).contiguous() if keep is not None else None, stream)


@pytest.mark.parametrize("F", [7, 128, 602])
@pytest.mark.parametrize("S", [1, 2, 3, 16])
@pytest.mark.parametrize("p", [0.0, 0.5, 1.0])
def test_coo_multi_equals_single_calls_bitwise(F, S, p):
    import torch
    from grand_plus_amd.augment import random_prop, sample_seed
    feats, scores, idx, g = ragged_coo(F, seed=F + 100 * S + int(10 * p), n_out=50)
    f, sc, ix = feats.cuda(), scores.cuda(), idx.cuda()
    n_out = int(idx[-1]) + 1
    seed = 0x1234567 + F * S
    out = _coo_multi(f, sc, ix, n_out, S, p, True, seed=seed)
    assert out.shape == (S, n_out, F)
    for s in range(S):
        one = random_prop(f, sc, ix, p, training=True, seed=sample_seed(seed, s))
        assert torch.equal(out[s], one), f"sample {s} differs from the single call with sample_seed"
    keep = (torch.rand((S, idx.numel()), generator=g) >= p).to(torch.uint8).cuda()
    out = _coo_multi(f, sc, ix, n_out, S, p, True, keep=keep)
    for s in range(S):
        assert torch.equal(out[s], random_prop(f, sc, ix, p, training=True, keep=keep[s].contiguous()))
    if S > 1:                                                                     # eval mode: every sample is the plain average
        out = _coo_multi(f, sc, ix, n_out, S, p, False, seed=seed)
        one = random_prop(f, sc, ix, p, training=False, seed=seed)
        for s in range(S):
            assert torch.equal(out[s], one)


@pytest.mark.parametrize("F", [7, 128, 602])
@pytest.mark.parametrize("S", [1, 2, 3, 16])
@pytest.mark.parametrize("p", [0.0, 0.5, 1.0])
def test_rows_multi_equals_single_calls_bitwise(F, S, p):
    import torch
    from grand_plus_amd import augment
    col, val, filled, X, g = rows_case(seed=F + S, F=F, empty_row=8)
    S_rows, K = col.shape
    rows = torch.randperm(S_rows, generator=g)[:90].to(torch.int32)
    rows[:2] = torch.tensor([5, 8], dtype=torch.int32)
    c, v, fl, x, r = col.reshape(-1).cuda(), val.reshape(-1).cuda(), filled.cuda(), X.cuda(), rows.cuda()
    seed = 0xABCDEF + F * S
    stream = torch.cuda.current_stream().cuda_stream

    def multi(training, seed=None, keep=None):
        if S > 1:
            return augment.random_prop_rows(x, c, v, fl, K, batch_rows=r, dropnode_rate=p, training=training, seed=seed,
                                            keep=keep, samples=S)
        return augment._rows_multi_forward(x, c, v, fl, K, r, r.numel(), 1, p, training, seed if seed is not None else 3,
                                           keep, stream)

    out = multi(True, seed=seed)
    assert out.shape == (S, rows.numel(), F)
    for s in range(S):
        one = augment.random_prop_rows(x, c, v, fl, K, batch_rows=r, dropnode_rate=p, training=True, seed=augment.sample_seed(seed, s))
        assert torch.equal(out[s], one), f"sample {s} differs from the single call with sample_seed"
    keep = (torch.rand((S, S_rows * K), generator=g) >= p).to(torch.uint8).cuda()
    out = multi(True, keep=keep)
    for s in range(S):
        one = augment.random_prop_rows(x, c, v, fl, K, batch_rows=r, dropnode_rate=p, training=True, keep=keep[s].contiguous())
        assert torch.equal(out[s], one)
    assert torch.count_nonzero(out[:, 1]) == 0                                      # the empty row
    if S > 1:
        out = multi(False, seed=seed)
        one = augment.random_prop_rows(x, c, v, fl, K, batch_rows=r, dropnode_rate=p, training=False)
        for s in range(S):
            assert torch.equal(out[s], one)


@pytest.mark.parametrize("F", [7, 128, 602])
@pytest.mark.parametrize("S", [2, 3, 16])
@pytest.mark.parametrize("training", [False, True])
def test_coo_multi_backward_matches_reference_gradient(F, S, training):
    import torch
    from grand_plus_amd.augment import random_prop
    p = 0.5
    feats, scores, idx, g = ragged_coo(F, seed=3 * F + S + training, n_out=50)
    keep = (torch.rand((S, idx.numel()), generator=g) >= p).to(torch.uint8)
    n_out = int(idx[-1]) + 1
    G = torch.randn((S, n_out, F), generator=g)
    ref, terms = ref_grad(feats, scores, idx, p, training, keep, G)
    x = feats.cuda().requires_grad_(True)
    out = random_prop(x, scores.cuda(), idx.cuda(), p, training=training, keep=keep.cuda(), samples=S)
    assert out.grad_fn is not None
    out.backward(G.cuda())
    close(x.grad, ref, terms)
    if training:                                                                  # dropped in every sample: exact zeros
        assert torch.count_nonzero(x.grad.cpu()[(keep == 0).all(0)]) == 0


@pytest.mark.parametrize("F", [7, 128, 602])
@pytest.mark.parametrize("S", [2, 3, 16])
@pytest.mark.parametrize("training", [False, True])
def test_rows_multi_backward_matches_reference_gradient(F, S, training):
    import torch
    from grand_plus_amd.augment import random_prop_rows
    col, val, filled, X, g = rows_case(seed=5 * F + S, F=F, empty_row=8)
    S_rows, K = col.shape
    rows = torch.randperm(S_rows, generator=g)[:90].to(torch.int32)
    rows[:2] = torch.tensor([5, 8], dtype=torch.int32)
    p = 0.5
    keep = (torch.rand((S, S_rows, K), generator=g) >= p).to(torch.uint8)
    idx, cols, scores, kp = rows_to_coo(col, val, filled, K, rows, keep)
    G = torch.randn((S, rows.numel(), F), generator=g)
    ref, terms = ref_grad(X, scores, idx, p, training, kp, G, cols=cols)
    x = X.cuda().requires_grad_(True)
    out = random_prop_rows(x, col.reshape(-1).cuda(), val.reshape(-1).cuda(), filled.cuda(), K, batch_rows=rows.cuda(),
                           dropnode_rate=p, training=training, keep=keep.reshape(S, -1).cuda(), samples=S)
    out.backward(G.cuda())
    close(x.grad, ref, terms)
    assert float(x.grad[7].abs().sum()) > 0


def test_coo_multi_with_n_out_needs_no_host_synchronisation():
    import torch
    from grand_plus_amd.augment import random_prop
    feats, scores, idx, g = ragged_coo(64, seed=11, n_out=50, long_row=False)
    n_out = int(idx[-1]) + 1
    x = feats.cuda().requires_grad_(True)
    sc, ix = scores.cuda(), idx.cuda()
    G = torch.randn((2, n_out, 64), generator=g).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = random_prop(x, sc, ix, 0.5, training=True, seed=99, samples=2, n_out=n_out)
        out.backward(G)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert out.shape == (2, n_out, 64)
    ref = random_prop(x.detach(), sc, ix, 0.5, training=True, seed=99, samples=2)   # n_out from the host read
    assert torch.equal(out.detach(), ref)
