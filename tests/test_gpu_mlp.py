"""The S-sample MLP block against the float64 restatement in oracle/mlp_ref.py of the reference's MLP.forward
(model.py:48-66 and model_mag.py:57-67) through torch autograd with F.batch_norm and the same keep masks, one call per
sample as the reference makes.  Tolerances in the style of §7e: outputs within 2e-5 * sum|a*w| (+1e-6) of the
last layer, gradients within 1e-4 of the largest reference entry."""
import numpy as np
import pytest

from augment_cases import rows_to_coo
from mlp_block_cases import hashed_keep, model_assert_grad, model_assert_out
from oracle.mlp_ref import RefMagMLP, RefMLP
from oracle.objective_ref import grand_loss_ref

pytestmark = pytest.mark.gpu

# (name, layout, F, H, C, nlayers, use_bn, node_norm, input_dropout, hidden_dropout, B): the run_*.sh shapes, plus a
# three-layer one at F = 7 and a MAG layout with BatchNorm
CASES = [
    ("cora", "model", 1433, 64, 7, 2, False, False, 0.5, 0.7, 150),
    ("citeseer", "model", 3703, 256, 6, 2, False, False, 0.0, 0.0, 250),
    ("pubmed", "model", 500, 16, 3, 1, True, True, 0.2, 0.2, 2),
    ("reddit", "model", 602, 512, 41, 2, True, True, 0.0, 0.0, 250),
    ("amazon2m", "model", 100, 1024, 47, 2, True, True, 0.0, 0.0, 250),
    ("aminer", "model", 100, 32, 18, 1, True, False, 0.0, 0.0, 1000),
    ("deep", "model", 7, 100, 5, 3, True, True, 0.3, 0.4, 150),
    ("mag", "mag", 64, 64, 8, 2, False, False, 0.0, 0.2, 150),
    ("mag_bn", "mag", 64, 64, 8, 3, True, True, 0.0, 0.2, 250),
]


def _pair(case, seed=0):
    """(ours on cuda, the restatement in float64 on cuda), same parameters and running statistics."""
    import torch
    from grand_plus_amd.mlp import GrandPlusMLP, MagMLP
    _, layout, F, H, C, nl, bn, norm, pin, phid, _B = case
    torch.manual_seed(seed)
    ours = (GrandPlusMLP if layout == "model" else MagMLP)(F, C, H, nl, bn, pin, phid, norm)
    g = torch.Generator().manual_seed(seed + 1)
    for b in ours.bns:                                       # non-trivial affine maps and running statistics
        b.weight.data = torch.rand(b.weight.shape, generator=g) + 0.5
        b.bias.data = torch.randn(b.bias.shape, generator=g) * 0.1
        b.running_mean.data = torch.randn(b.running_mean.shape, generator=g) * 0.1
        b.running_var.data = torch.rand(b.running_var.shape, generator=g) + 0.5
    ref = (RefMLP if layout == "model" else RefMagMLP)(F, C, H, nl, bn, pin, phid, norm)
    ref.load_state_dict(ours.state_dict())
    return ours.cuda(), ref.double().cuda()


def _keeps(ours, S, B, g):
    import torch
    mag = hasattr(ours, "embeds")
    ps = [ours.hidden_droprate if (mag or i > 0) else ours.input_droprate for i in range(len(ours.fcs))]
    return [(torch.rand((S, B, fc.weight.shape[1]), generator=g) >= p).to(torch.uint8).cuda() for fc, p in zip(ours.fcs, ps)]


def _run_ref(ref, X64, keeps):
    """The restatement, once per sample: (out [S, B, C], last-layer inputs [S, B, K])."""
    import torch
    outs, lasts = [], []
    for s in range(X64.shape[0]):
        outs.append(ref(X64[s], [k[s] for k in keeps]))
        lasts.append(ref.last_a)
    return torch.stack(outs), torch.stack(lasts)


_assert_out, _assert_grad = model_assert_out, model_assert_grad       # the rule of this file, stated in mlp_block_cases


@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_forward_gradients_and_running_stats_match_the_float64_restatement(case, S):
    import torch
    ours, ref = _pair(case)
    B, F = case[-1], case[2]
    g = torch.Generator().manual_seed(7)
    X = torch.randn((S, B, F), generator=g)
    if case[1] == "model" and F > 100:
        X = X * (torch.rand((S, B, F), generator=g) < 0.1)                    # sparse rows, bag-of-words like
    X = X.cuda()
    keeps = _keeps(ours, S, B, g)
    ours.train(); ref.train()
    Xo = X.clone().requires_grad_(True)
    out = ours(Xo, keep=keeps)
    X64 = X.double().requires_grad_(True)
    ref_out, last_a = _run_ref(ref, X64, keeps)
    _assert_out(out, ref_out, last_a, ref.fcs[-1])
    gy = torch.randn(out.shape, generator=g).cuda()
    out.backward(gy)
    ref_out.backward(gy.double())
    for (name, p), (_, q) in zip(ours.named_parameters(), ref.named_parameters()):
        if q.grad is None:                                    # unused: BatchNorm off
            assert p.grad is None, name
            continue
        if name == "fcs.0.bias" and case[1] == "model" and case[6] and not case[7] and len(ours.fcs) > 1:
            continue                                          # cancelled by the next BatchNorm: 0 up to rounding on both sides
        _assert_grad(p.grad, q.grad, name)
    if case[1] == "model" and case[7]:                        # layer 0's node_norm is detached: X gets no gradient
        assert Xo.grad is None
    else:
        _assert_grad(Xo.grad, X64.grad, "X")
    for (name, b), (_, rb) in zip(ours.named_buffers(), ref.named_buffers()):
        if name.endswith("num_batches_tracked"):
            assert int(b) == (S if case[6] else 0), name
        else:
            torch.testing.assert_close(b.double(), rb, rtol=1e-5, atol=1e-6, msg=name)


def test_running_stats_equal_s_sequential_batchnorm_calls():
    """After one S-sample call, running_mean / running_var / num_batches_tracked are those of S nn.BatchNorm1d calls."""
    import torch
    from grand_plus_amd.mlp import GrandPlusMLP
    S, B, F = 4, 150, 602
    torch.manual_seed(3)
    m = GrandPlusMLP(F, 9, 32, 2, True, 0.0, 0.0, False).cuda().train()
    bns = [torch.nn.BatchNorm1d(b.num_features).double().cuda().train() for b in m.bns]
    X = torch.randn((S, B, F), device="cuda") * 2 + 0.5
    with torch.no_grad():
        m(X)
        for s in range(S):
            h = bns[0](X[s].double())
            h = torch.nn.functional.linear(h, m.fcs[0].weight.double(), m.fcs[0].bias.double())
            bns[1](torch.relu(h))
    for ob, rb in zip(m.bns, bns):
        torch.testing.assert_close(ob.running_mean.double(), rb.running_mean, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(ob.running_var.double(), rb.running_var, rtol=1e-5, atol=1e-6)
        assert int(ob.num_batches_tracked) == int(rb.num_batches_tracked) == S


@pytest.mark.parametrize("layout", ["model", "mag"])
def test_sample_independence_bitwise(layout):
    """out[s] is bit for bit the S = 1 call with sample_seed(seed, s), and with keep[s]; in eval, the [B, F] call."""
    import torch
    from grand_plus_amd.augment import sample_seed
    case = ("deep", layout, 64 if layout == "mag" else 300, 100, 5, 3, True, True, 0.3, 0.4, 150)
    ours, _ = _pair(case)
    S, B = 4, 150
    g = torch.Generator().manual_seed(2)
    X = torch.randn((S, B, case[3] if layout == "mag" else case[2]), generator=g).cuda()     # MAG's input is the embedding
    ours.train()
    seed = 0x1234_5678_9ABC
    with torch.no_grad():
        out = ours(X, seed=seed)
        for s in range(S):
            one = ours(X[s:s + 1].contiguous(), seed=sample_seed(seed, s))
            assert torch.equal(one[0], out[s]), s
        keeps = _keeps(ours, S, B, g)
        out = ours(X, keep=keeps)
        for s in range(S):
            one = ours(X[s:s + 1].contiguous(), keep=[k[s:s + 1].contiguous() for k in keeps])
            assert torch.equal(one[0], out[s]), s
        ours.eval()
        out = ours(X)
        for s in range(S):
            assert torch.equal(ours(X[s]), out[s])


def test_hashed_dropout_keeps_one_minus_p_and_follows_the_seed():
    import torch
    from grand_plus_amd.mlp import GrandPlusMLP
    torch.manual_seed(0)
    F, B = 300, 250
    m = GrandPlusMLP(F, 3, 8, 1, False, 0.5, 0.0, False).cuda().train()
    X = torch.ones((1, B, F), device="cuda")
    with torch.no_grad():
        a, b, c = m(X, seed=99), m(X, seed=99), m(X, seed=100)
    assert torch.equal(a, b) and not torch.equal(a, c)
    # no node_norm, no BN: dX = keep / (1 - p) * W^T 1, with W all ones and C = 3
    Xg = X.clone().requires_grad_(True)
    m.fcs[0].weight.data.fill_(1.0)
    m(Xg, seed=99).sum().backward()
    kept = Xg.grad != 0
    assert abs(float(kept.double().mean()) - 0.5) < 0.01
    assert bool((Xg.grad[kept] == 6.0).all())


def test_determinism_bitwise():
    import torch
    case = CASES[3]                                          # reddit: BN, node_norm
    runs = []
    for _ in range(2):
        ours, _ = _pair(case)
        ours.train()
        g = torch.Generator().manual_seed(4)
        X = torch.randn((2, 250, case[2]), generator=g).cuda()
        out = ours(X, seed=77)
        out.backward(torch.randn(out.shape, generator=g).cuda())
        runs.append([out.detach().clone()] + [p.grad.clone() for p in ours.parameters()] + [b.clone() for b in ours.buffers()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_eval_mode_10000_rows_and_above_65535_rows():
    import torch
    for case, B in ((CASES[3], 10000), (CASES[4], 70000)):
        ours, ref = _pair(case)
        ours.eval(); ref.eval()
        X = torch.randn((B, case[2]), device="cuda")
        with torch.no_grad():
            out = ours(X)
            ref_out = ref(X.double(), [None] * 3)
        assert out.shape == (B, case[4])
        _assert_out(out, ref_out, ref.last_a, ref.fcs[-1])


def test_dropout_edges_p0_p1_and_no_bn():
    import torch
    for pin, phid in ((0.0, 0.0), (1.0, 0.5), (0.5, 1.0)):
        case = ("edge", "model", 120, 40, 6, 2, False, True, pin, phid, 64)
        ours, ref = _pair(case)
        ours.train(); ref.train()
        g = torch.Generator().manual_seed(5)
        X = torch.randn((2, 64, 120), generator=g).cuda()
        keeps = _keeps(ours, 2, 64, g)
        out = ours(X, keep=keeps)
        ref_out, last_a = _run_ref(ref, X.double(), keeps)
        _assert_out(out, ref_out, last_a, ref.fcs[-1])
        if phid == 1.0:                                        # the last layer sees zeros: the output is its bias
            assert torch.equal(out, ours.fcs[1].bias.detach().expand_as(out))
        out.sum().backward()
        assert all(bool(torch.isfinite(p.grad).all()) for p in ours.parameters() if p.grad is not None)
        with torch.no_grad():                                  # the hash path at the same edges
            assert bool(torch.isfinite(ours(X, seed=3)).all())


def test_state_dict_round_trips_with_the_restatement():
    import torch
    from grand_plus_amd.mlp import GrandPlusMLP, MagMLP
    for ours_cls, ref_cls in ((GrandPlusMLP, RefMLP), (MagMLP, RefMagMLP)):
        for nl in (1, 2, 3):
            a, b = ours_cls(30, 4, 16, nl, True, 0.1, 0.2, True), ref_cls(30, 4, 16, nl, True, 0.1, 0.2, True)
            assert list(a.state_dict()) == list(b.state_dict())
            b.load_state_dict(a.state_dict())
            a2 = ours_cls(30, 4, 16, nl, True, 0.1, 0.2, True)
            a2.load_state_dict(b.state_dict())
            for k, v in a.state_dict().items():
                assert torch.equal(v, a2.state_dict()[k])


def test_forward_and_backward_do_not_synchronise():
    import torch
    case = CASES[3]
    ours, _ = _pair(case)
    ours.train()
    X = torch.randn((2, 250, case[2]), device="cuda")
    gy = torch.randn((2, 250, case[4]), device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = ours(X, seed=5)
        out.backward(gy)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert all(p.grad is not None for p in ours.parameters())
    # the reference step's torch path does synchronise there (consis_loss's boolean-mask indexing, model.py:134), so the
    # mode is live on this build
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            lps = [torch.log_softmax(ours.reference_forward(X[s]), -1) for s in range(2)]
            avg = (lps[0].exp() + lps[1].exp()) / 2
            lps[0][avg.max(1)[0] > 0.05].sum()
    finally:
        torch.cuda.set_sync_debug_mode(0)


# ---- steps end to end
def _check_params(ours, ref):
    for (name, p), (_, q) in zip(ours.named_parameters(), ref.named_parameters()):
        if q.grad is None:
            assert p.grad is None, name
            continue
        _assert_grad(p.grad, q.grad, name)


@pytest.mark.parametrize("shape", ["cora", "reddit"])
def test_training_step_end_to_end(shape):
    """gfpush_device -> batch_positions -> random_prop_rows(samples=2) -> GrandPlusMLP -> grand_plus_loss -> backward,
    every parameter gradient against the float64 pipeline under the same masks."""
    import torch
    from grand_plus_amd import Graph, synth
    from grand_plus_amd.augment import random_prop_rows
    from grand_plus_amd.objective import grand_plus_loss
    from grand_plus_amd.recipes import make_coef
    from grand_plus_amd.rows import RowMatrix
    from oracle.random_prop_ref import random_prop_ref
    case = CASES[0] if shape == "cora" else CASES[3]
    F, C = case[2], case[4]
    n_l, n_u = (50, 100) if shape == "cora" else (50, 200)
    B, K, S, p_node = n_l + n_u, 32, 2, 0.5
    indptr, indices = synth.shape_csr("tiny")
    n = len(indptr) - 1
    seeds = synth.seeds(n, 400)
    g = Graph(indptr, indices, 0)
    rm = RowMatrix.compute(g, seeds, make_coef("ppr", 6, 0.2), 1e-5, K)
    gen = torch.Generator().manual_seed(1)
    X = (torch.rand((n, F), generator=gen) < 0.05).float() if shape == "cora" else torch.randn((n, F), generator=gen)
    batch_nodes = torch.from_numpy(np.asarray(seeds[:B], dtype=np.int64))
    labels = torch.randint(0, C, (n_l,), generator=gen)
    keep = (torch.rand((S, len(seeds) * K), generator=gen) >= p_node).to(torch.uint8)
    ours, ref = _pair(case, seed=11)
    ours.train(); ref.train()
    keeps = _keeps(ours, S, B, gen)
    w, tem = 0.8, 0.5

    rows = rm.batch_positions(batch_nodes.cuda(), check=False)
    aug = random_prop_rows(X.cuda(), rm.col, rm.val, rm.filled, K, batch_rows=rows, dropnode_rate=p_node, training=True,
                           keep=keep.cuda(), samples=S)
    loss, _ = grand_plus_loss(ours(aug, keep=keeps), labels.cuda(), n_l, w, tem=tem, conf=0.0, kind="l2")
    loss.backward()

    idx, cols, scores, kp = rows_to_coo(rm.col.cpu(), rm.val.cpu(), rm.filled.cpu(), K, rows.cpu(), keep)
    aug_r = torch.stack([random_prop_ref(X.double()[cols], scores.double(), idx, p_node, True, kp[s]) for s in range(S)]).cuda()
    z_ref, _ = _run_ref(ref, aug_r, keeps)
    loss_r, _, _ = grand_loss_ref(z_ref, labels.cuda(), n_l, w, tem, 0.0, "l2")   # every unlabelled row in the consistency term
    loss_r.backward()
    assert abs(float(loss) - float(loss_r)) <= 1e-4 * abs(float(loss_r)) + 1e-6, (float(loss), float(loss_r))
    _check_params(ours, ref)


def test_mag_shaped_step_through_magmlp_reaches_the_embedding_table():
    """§7d's MAG-shaped step: embedding_bag_csr -> random_prop(samples=2) -> MagMLP -> grand_plus_loss -> backward; the
    gradient reaches the embedding table."""
    import scipy.sparse as sp
    import torch
    from grand_plus_amd import Graph, synth
    from grand_plus_amd.augment import random_prop
    from grand_plus_amd.embedding import flatten_rows
    from grand_plus_amd.mlp import MagMLP
    from grand_plus_amd.objective import grand_plus_loss
    from grand_plus_amd.recipes import make_coef
    from oracle.random_prop_ref import random_prop_ref
    indptr, indices = synth.shape_csr("tiny")
    n = len(indptr) - 1
    seeds = synth.seeds(n, 300)
    K, H, C, V, p_node, S = 32, 64, 8, 900, 0.5, 2
    g = Graph(indptr, indices, 0)
    _, col, val, filled = g.gfpush_device(torch.from_numpy(seeds).cuda(), make_coef("ppr", 6, 0.2), 1e-5, K)
    rng = np.random.default_rng(5)
    A = sp.random(n, V, density=0.02, format="csr", random_state=rng, dtype=np.float32)
    A.data = (A.data + 0.05).astype(np.float32)
    ip = torch.from_numpy(A.indptr.astype(np.int64)).cuda()
    ix = torch.from_numpy(A.indices.astype(np.int32)).cuda()
    dt = torch.from_numpy(A.data).cuda()
    torch.manual_seed(0)
    ours = MagMLP(V, C, H, 2, False, 0.0, 0.2, False)
    ref = RefMagMLP(V, C, H, 2, False, 0.0, 0.2, False)
    ref.load_state_dict(ours.state_dict())
    ours.cuda().train(); ref.double().cuda().train()
    batch_rows = torch.arange(0, 40, dtype=torch.int32).cuda()                  # 20 labelled + 20 unlabelled (run_mag.sh)
    n_train, n_out = 20, 40
    gen = torch.Generator().manual_seed(0)
    labels = torch.randint(0, C, (n_train,), generator=gen)
    nbr, scores, mat_idx = flatten_rows(col, val, filled, K, batch_rows)
    M = nbr.numel()
    keep = (torch.rand((S, M), generator=gen) >= p_node).to(torch.uint8)
    keeps = _keeps(ours, S, n_out, gen)

    emb = ours.emb_csr(ip, ix, dt, nodes=nbr)
    aug = random_prop(emb, scores, mat_idx, p_node, training=True, keep=keep.cuda(), samples=S, n_out=n_out)
    loss, _ = grand_plus_loss(ours(aug, keep=keeps), labels.cuda(), n_train, 1.0, tem=0.5, conf=0.0, kind="l2")
    loss.backward()

    sub = A[nbr.cpu().numpy()]
    node_idx, attr_idx = sub.nonzero()
    node_idx = torch.from_numpy(node_idx.astype(np.int64)).cuda()
    attr_idx = torch.from_numpy(attr_idx.astype(np.int64)).cuda()
    data = torch.from_numpy(sub.data).double().cuda()
    Wr = ref.embeds.weight
    num = torch.zeros((M, H), dtype=torch.float64, device="cuda").index_add_(0, node_idx, Wr[attr_idx] * data[:, None])
    den = torch.zeros((M, 1), dtype=torch.float64, device="cuda").index_add_(0, node_idx, data[:, None])
    emb_r = num / (den + 1e-10)                                                  # MLP.emb, model_mag.py:48-55 (no dropout)
    aug_r = torch.stack([random_prop_ref(emb_r, scores.double(), mat_idx, p_node, True, keep[s].cuda()) for s in range(S)])
    z_ref, _ = _run_ref(ref, aug_r, keeps)
    loss_r, _, _ = grand_loss_ref(z_ref, labels.cuda(), n_train, 1.0, 0.5, 0.0, "l2")
    loss_r.backward()
    assert abs(float(loss) - float(loss_r)) <= 1e-4 * abs(float(loss_r)) + 1e-6
    assert float(ours.embeds.weight.grad.abs().max()) > 0
    _check_params(ours, ref)


def test_hashed_masks_are_the_mirrored_layer_seed_formula():
    """The hash path equals the explicit-mask path with masks recomputed on the host from mlp.layer_seed and
    augment.hip's counter hash (entry b * F + f)."""
    import torch
    from grand_plus_amd.mlp import GrandPlusMLP, layer_seed
    S, B = 3, 20
    torch.manual_seed(1)
    m = GrandPlusMLP(40, 5, 24, 3, True, 0.3, 0.6, True).cuda().train()
    seed = 0xDEADBEEF12345

    def mask(layer, F, p):                                   # the host mirror, shared with tests/test_gpu_mlp_block.py
        return hashed_keep(seed, layer, S, B, F, p).cuda()

    keeps = [mask(0, 40, 0.3), mask(1, 24, 0.6), mask(2, 24, 0.6)]
    X = torch.randn((S, B, 40), device="cuda")
    with torch.no_grad():
        assert torch.equal(m(X, seed=seed), m(X, keep=keeps))
