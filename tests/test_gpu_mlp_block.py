"""One MLP block of csrc/mlp.hip through the public `grand_plus_amd.mlp.block`, per case of
tests/mlp_block_cases.py, against the float64 twin run on the GPU: every flag set, S up to 16, the three GEMM
instantiations at their M, N, K and split edges, the BatchNorm and row kernels' tails, the optional pointers, dropout by
mask and by hash -- forward, every gradient and the running statistics, under that module's bounds.  Then the buffers:
guard bands behind every allocation and a NaN pattern under it at the shapes that fill the split-K workspaces to the last
float, and bitwise determinism of the backward at S = 16.  tests/test_host_mlp_block.py proves on the CPU that the bounds
leave float32 room and that the cases can fail.  Inputs are built on the CPU and copied."""
import math

import pytest
import torch

import mlp_block_cases as mc

pytestmark = pytest.mark.gpu


def _block(bd, x):
    from grand_plus_amd import mlp
    c = bd.case
    return mlp.block(x, bd.fc, bd.bn, relu=bool(c.flags & mc.RELU), node_norm=bool(c.flags & mc.NORM),
                     training=bool(c.flags & mc.TRAIN), dropout=c.p, seed=mc.DROP_SEED, layer=0,
                     keep=None if c.hashed else bd.keep)


def _run(bd):
    """Ours on a case that is on the GPU (its modules are used and its running statistics updated): a Ref without `a`."""
    c = bd.case
    x = bd.x.clone().requires_grad_("x" in c.rg)
    params = {"w": bd.fc.weight, "b": bd.fc.bias, "gamma": bd.bn.weight if bd.bn is not None else None,
              "beta": bd.bn.bias if bd.bn is not None else None}
    for name, p in params.items():
        if p is not None:
            p.requires_grad_(name in c.rg)
            p.grad = None
    out = _block(bd, x)
    out.backward(bd.gy)
    grad = lambda t: t.grad if t is not None else None  # noqa: E731
    bn = bd.bn
    return mc.Ref(out.detach(), None, x.grad, *(grad(params[k]) for k in ("w", "b", "gamma", "beta")),
                  bn.running_mean if bn is not None else None, bn.running_var if bn is not None else None,
                  int(bn.num_batches_tracked) if bn is not None else None)


def _check(c):
    b = mc.build(c)
    bd = mc.to(b, "cuda")
    ref = mc.block_ref64(bd)
    got = _run(bd)
    mc.assert_case(bd, got, ref)
    if bd.bn is not None and not c.flags & mc.TRAIN:         # eval leaves the running statistics alone
        assert torch.equal(got.rm.cpu(), b.bn.running_mean) and torch.equal(got.rv.cpu(), b.bn.running_var)
    return b, bd, got, ref


def _same(a, b, what):
    for name in ("out", "gx", "gw", "gb", "gg", "gbe", "rm", "rv"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert torch.equal(x, y), f"{what}: {name} differs in {int((x != y).sum())} places"
    assert a.nbt == b.nbt, what


@pytest.mark.parametrize("c", mc.FLAGS, ids=mc.ids(mc.FLAGS))
def test_every_flag_set(c):
    """All 16 of RELU, NORM, BN, TRAINING with every gradient wanted: eval-mode backward, NORM without BN or RELU, RELU|BN."""
    _check(c)


@pytest.mark.parametrize("c", mc.SAMPLES, ids=mc.ids(mc.SAMPLES))
def test_sample_counts_up_to_16_and_sample_independence(c):
    """Against float64, and out[s] and the running statistics bit for bit those of S calls with one sample each (forward
    only: dA's chunking depends on S B)."""
    b, bd, got, _ = _check(c)
    one = mc.to(b, "cuda")                                   # fresh running statistics, carried through the S calls
    with torch.no_grad():
        for s in range(c.S):
            part = mc.Built(c, one.x[s:s + 1].contiguous(), one.fc, one.bn, one.keep[s:s + 1].contiguous(), None)
            assert torch.equal(_block(part, part.x)[0], got.out[s]), f"sample {s}"
    if one.bn is not None:
        assert torch.equal(one.bn.running_mean, got.rm) and torch.equal(one.bn.running_var, got.rv)
        assert int(one.bn.num_batches_tracked) == got.nbt


@pytest.mark.parametrize("c", mc.GEMM_EDGES, ids=mc.ids(mc.GEMM_EDGES))
def test_gemm_tile_and_split_edges(c):
    """Flags T, p = 0: out, dX = dA and dW are the three GEMM instantiations alone, each walked over its M, N, K and its
    split counts (mlp_reduce_kernel, a last chunk of one element)."""
    _check(c)


@pytest.mark.parametrize("c", mc.BN_EDGES, ids=mc.ids(mc.BN_EDGES))
def test_batchnorm_column_kernel_tails(c):
    """The 16 x 16 column kernels' tails in B and F, with a column of zero variance and a zero column."""
    _check(c)


@pytest.mark.parametrize("c", mc.BN_HYPER, ids=mc.ids(mc.BN_HYPER))
def test_batchnorm_eps_and_momentum_away_from_the_defaults(c):
    """eps = 1e-3 and momentum = 0.3 in training: the normalised forward, its backward and both running statistics."""
    b, bd, _, _ = _check(c)
    assert bd.bn.eps == 1e-3 and bd.bn.momentum == 0.3 and b.bn.eps == 1e-3


@pytest.mark.parametrize("c", mc.ROW_EDGES, ids=mc.ids(mc.ROW_EDGES))
def test_row_kernel_tails_and_degenerate_rows(c):
    b, bd, got, _ = _check(c)
    if c.flags & mc.RELU:                                    # the row that ReLU zeroes: output = bias, dX row = 0, exactly
        assert torch.equal(got.out[0, 0], bd.fc.bias.detach()) and not bool(got.gx[0, 0].any())
        gx = got.gx.view(-1, c.F)                            # and no gradient through an entry that is -0.0 or 0.0
        assert not bool(gx[2, 0]) and not bool(gx[2, 1] if c.F >= 3 else gx[3, 0])


def test_norm_without_relu_over_a_zero_row():
    """node_norm of a zero row is 0 / 1e-12: dX = 1e12 * g * keep / (1 - p) there, g = dY W, in float64 torch and here.  That
    row would set the scale of the whole tensor, so it is checked by itself, relative to its own fma sum, and the other
    rows against the reference scaled by their own largest entry."""
    c = mc.ZERO_ROW
    bd = mc.to(mc.build(c), "cuda")
    ref = mc.block_ref64(bd)
    got = _run(bd)
    M, row = c.S * c.B, 4
    W, gy = bd.fc.weight.detach().double(), bd.gy.double().view(M, c.N)
    scale = bd.keep.view(M, c.F)[row].double() / (1.0 - c.p)
    want = 1e12 * scale * (gy @ W)[row]
    bound = 1e12 * scale * 2e-5 * (gy.abs() @ W.abs())[row]
    err = (got.gx.view(M, c.F)[row].double() - want).abs()
    print(f"[mlp_block] {c.name} zero row: err / bound {float((err / bound.clamp(min=1e-300)).max()):.3g}")
    assert bool((err <= bound).all()) and float(want.abs().max()) > 1e9
    rest = torch.arange(M, device="cuda") != row
    r = ref.gx.view(M, c.F)[rest]
    err = (got.gx.view(M, c.F)[rest].double() - r).abs() / (1e-5 * (r.abs() + r.abs().max()) + 1e-9)
    print(f"[mlp_block] {c.name} other rows: err / bound {float(err.max()):.3g}")
    assert float(err.max()) <= 1.0
    sh = mc.shares(bd, got, ref, only={"out", "gw", "gb"})
    assert all(v <= 1.0 for v in sh.values()), sh
    assert torch.equal(got.out.view(M, c.N)[row], bd.fc.bias.detach())


@pytest.mark.parametrize("c", mc.OPTIONAL, ids=mc.ids(mc.OPTIONAL))
def test_optional_pointers(c):
    """No bias, BatchNorm without affine parameters, and the requires_grad patterns that leave d_grad_x, d_grad_weight or
    the BatchNorm gradients NULL: what exists matches, what should not exist is None (assert_case)."""
    _check(c)


@pytest.mark.parametrize("c", mc.DROPOUT, ids=mc.ids(mc.DROPOUT))
def test_dropout_edges_by_mask_and_by_hash(c):
    """p = 0, p = 1 and the hashed p = 0.5 against the mask recomputed on the host, gradients included."""
    b, bd, got, _ = _check(c)
    if c.p == 1.0:
        assert torch.equal(got.out, bd.fc.bias.detach().expand_as(got.out)) and not bool(got.gx.any())
    if c.hashed and c.p == 0.5:                              # the hash is live: another seed gives another result
        other = mc.to(b, "cuda")
        from grand_plus_amd import mlp
        with torch.no_grad():
            out = mlp.block(other.x, other.fc, other.bn, relu=bool(c.flags & mc.RELU), node_norm=bool(c.flags & mc.NORM),
                            training=True, dropout=c.p, seed=mc.DROP_SEED + 1, layer=0)
        assert not torch.equal(out, got.out)


def test_backward_is_bitwise_deterministic_at_16_samples():
    c = next(c for c in mc.SAMPLES if c.S == 16 and c.flags == mc.FULL)
    b = mc.build(c)
    _same(_run(mc.to(b, "cuda")), _run(mc.to(b, "cuda")), c.name)


# ---- the buffers
PATTERN = 0x7FA5A5A5                                         # a NaN as float32
TAIL_WORDS = 1024                                            # 4 KiB behind every allocation


class _Guarded:
    """torch.empty / torch.empty_like for CUDA requests: the request plus a 4 KiB tail, all of it filled with PATTERN; the
    caller gets a tensor over the leading bytes and the parent is remembered."""

    def __init__(self):
        self.real_empty, self.real_empty_like = torch.empty, torch.empty_like
        self.allocs = []                                     # (parent int32, tensor, bytes)

    def empty(self, *size, dtype=None, device=None, **kw):
        if kw or device is None or torch.device(device).type != "cuda":
            return self.real_empty(*size, dtype=dtype, device=device, **kw)
        if len(size) == 1 and not isinstance(size[0], int):
            size = tuple(size[0])
        dtype = dtype or torch.get_default_dtype()
        nbytes = math.prod(size) * self.real_empty(0, dtype=dtype).element_size()
        parent = self.real_empty((nbytes + 3) // 4 + TAIL_WORDS, dtype=torch.int32, device=device).fill_(PATTERN)
        t = self.real_empty(0, dtype=dtype, device=device).set_(parent.untyped_storage(), 0, size)
        self.allocs.append((parent, t, nbytes))
        return t

    def empty_like(self, t, **kw):
        if kw or not t.is_cuda:
            return self.real_empty_like(t, **kw)
        return self.empty(tuple(t.shape), dtype=t.dtype, device=t.device)


def _saved_written(c):
    """Which floats of `saved` ([S B] row scales, then mean, invstd, mul, add of [S x F] each) the flags say are written."""
    M, n = c.S * c.B, c.S * c.F
    w = torch.zeros(M + 4 * n, dtype=torch.bool)
    if c.flags & mc.NORM:
        w[:M] = True
    if c.flags & mc.BN:
        for part in range(4):                                # every sample's slot in training, slot 0 in eval
            w[M + part * n:M + part * n + (n if c.flags & mc.TRAIN else c.F)] = True
    return w


@pytest.mark.parametrize("c", mc.GUARD, ids=mc.ids(mc.GUARD))
def test_kernels_stay_inside_their_buffers_and_write_all_of_them(c, monkeypatch):
    """block() and its backward over guarded allocations (no pointer is assembled here): every tail intact, no pattern
    left in out, saved_a, the written parts of saved or any gradient, and the bits of the unguarded call.  Three of the
    shapes fill the forward workspace, dA's partials and dW's partials to the last float."""
    b, bd, plain, _ = _check(c)
    g = _Guarded()
    gd = mc.to(b, "cuda")
    with monkeypatch.context() as m:
        m.setattr(torch, "empty", g.empty)
        m.setattr(torch, "empty_like", g.empty_like)
        got = _run(gd)
    torch.cuda.synchronize()
    names = ["out", "saved", "saved_a", "forward workspace", "gx", "gw", "gb", "gg", "gbe", "backward workspace"]
    assert len(g.allocs) == len(names), [tuple(t.shape) for _, t, _ in g.allocs]
    for name, (parent, t, nbytes) in zip(names, g.allocs):
        raw = parent.view(torch.uint8)
        fresh = torch.full_like(parent, PATTERN).view(torch.uint8)
        assert raw.numel() - nbytes >= 4 * TAIL_WORDS and torch.equal(raw[nbytes:], fresh[nbytes:]), f"{name}: written past its end"
        if t.dtype != torch.float32:
            assert "workspace" in name
            continue
        untouched = parent[:t.numel()] == PATTERN
        if name == "saved":
            assert t.numel() == c.S * c.B + 4 * c.S * c.F
            untouched &= _saved_written(c).to(untouched.device)
        assert not bool(untouched.any()), f"{name}: {int(untouched.sum())} of {t.numel()} elements never written"
    assert g.allocs[0][1].data_ptr() == got.out.data_ptr()                  # the guarded buffers are the ones in use
    _same(got, plain, c.name)
