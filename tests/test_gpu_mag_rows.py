"""MAG's fused front end on the GPU: `mag_prop_rows` forward and `weight.grad` against the float64
restatement of tests/mag_cases.py under §7d's rule, the bitwise claims of its order contract, its bounds rules, parity
with the composed path (flatten_rows -> embedding_bag_csr -> random_prop) through a whole MAG-shaped training step, the
absence of host synchronisation, and `valid_mag` / `predict_mag`.  Every case is tiny."""
import numpy as np
import pytest
import torch

import evaluate_cases as ec
import mag_cases as mc

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _cuda(t):
    return None if t is None else t.cuda()


def _run(c, W=None, batch="case", **over):
    """mag_prop_rows on the tensors of case c (dict of mag_cases.case), its keywords overridden by `over`: [S, B, H]."""
    from grand_plus_amd import mag_prop_rows
    w, ip, ix, dt, col, val, filled, K = c["P"].cuda()
    kw = dict(c["kw"])
    kw.update(over)
    out = mag_prop_rows(w if W is None else W, ip, ix, dt, col, val, filled, K, _cuda(c["batch"] if isinstance(batch, str) else batch), **kw)
    return out[None] if kw["samples"] == 1 else out


# ------------------------------------------------------------------------------------------ against the float64 reference
@pytest.mark.parametrize("name", list(mc.CASES))
def test_forward_and_weight_gradient_match_float64(name):
    """Explicit DropNode mask, the hashed input-dropout mask rebuilt on the host by the reference."""
    c = mc.case(name)
    out64, terms, dW64, dW_terms = c["ref"]
    W = c["P"].W.cuda().requires_grad_(True)
    out = _run(c, W=W, keep=_cuda(c["keep"]))
    assert out.shape == out64.shape and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    r_out = mc.close(out.detach(), out64, terms, c["roundings"], f"{name} forward")
    (out * c["G"].cuda()).sum().backward()
    assert W.grad is not None and bool(torch.isfinite(W.grad).all())
    r_grad = mc.close(W.grad, dW64, dW_terms, c["roundings"], f"{name} dW")
    print(f"[mag] {name}: error / bound forward {r_out:.3g}, dW {r_grad:.3g}")
    if c["kw"]["dropnode_rate"] == 1.0 or c["kw"]["input_droprate"] == 1.0:
        assert not bool(out.any()) and not bool(W.grad.any())                      # p = 1 gives zeros


@pytest.mark.parametrize("name", ["h7_k5_s3", "h64_k32_s2", "pin05_s16"])
def test_the_hashed_dropnode_mask_is_the_mirrored_formula(name):
    c = mc.case(name)
    P = c["P"]
    keep = mc.node_keep(mc.SEED, c["S"], P.S_rows * P.K, c["kw"]["dropnode_rate"])
    assert 0 < int(keep.sum()) < keep.numel()
    assert _same(_run(c), _run(c, keep=keep.cuda()))


def test_the_hashed_dropnode_mask_is_random_prop_rows_mask_for_the_same_seed():
    """Identity tables on both sides: out[s, b, n] != 0 exactly where the slot of row b that holds node n was kept."""
    from grand_plus_amd import mag_prop_rows
    from grand_plus_amd.augment import random_prop_rows
    N, K, S_rows, S, seed = 40, 8, 12, 3, 0xABCDEF
    g = torch.Generator().manual_seed(3)
    col = torch.stack([torch.randperm(N, generator=g)[:K] for _ in range(S_rows)]).to(torch.int32).reshape(-1).cuda()
    val = (torch.rand((S_rows * K,), generator=g, dtype=torch.float64) + 0.1).cuda()
    filled = torch.full((S_rows,), K, dtype=torch.int32).cuda()
    eye = torch.eye(N).cuda()
    ip = torch.arange(N + 1, dtype=torch.int64).cuda()
    ix = torch.arange(N, dtype=torch.int32).cuda()
    dt = torch.ones(N).cuda()
    a = mag_prop_rows(eye, ip, ix, dt, col, val, filled, K, samples=S, dropnode_rate=0.5, seed=seed)
    b = random_prop_rows(eye, col, val, filled, K, dropnode_rate=0.5, seed=seed, samples=S)
    kept = int((a != 0).sum())
    assert torch.equal(a != 0, b != 0) and 0 < kept < S * S_rows * K
    assert not torch.equal(a[0] != 0, a[1] != 0)


# ------------------------------------------------------------------------------------------------------- bitwise claims
@pytest.mark.parametrize("name", ["h7_k5_s3", "h64_k32_s2", "h65_k5_s16", "h130_k32_s3", "pin05_h65_s3", "pin05_h64_k32", "pin05_s16"])
def test_sample_s_equals_the_single_sample_call_bit_for_bit(name):
    from grand_plus_amd._common import sample_seed
    c = mc.case(name)
    keep = c["keep"].cuda()
    hashed, masked = _run(c), _run(c, keep=keep)
    assert _same(hashed, _run(c)) and _same(masked, _run(c, keep=keep))            # the forward is the same run to run
    for s in range(c["S"]):
        seed_s = sample_seed(mc.SEED, s)                                           # (also the input mask's seed of sample s)
        assert _same(hashed[s], _run(c, samples=1, seed=seed_s)[0]), s
        assert _same(masked[s], _run(c, samples=1, seed=seed_s, keep=keep[s].contiguous())[0]), s


@pytest.mark.parametrize("name", ["pin0_pnode0", "h7_k5_s3"])
def test_eval_mode_equals_training_at_rate_zero(name):
    c = mc.case(name)
    assert _same(_run(c, training=False, dropnode_rate=0.5, input_droprate=0.5), _run(c, training=True, dropnode_rate=0.0, input_droprate=0.0))


# --------------------------------------------------------------------------------------------------------------- bounds
def test_out_of_range_ids_are_skipped_counted_and_leave_the_other_rows_alone():
    from grand_plus_amd import mag_prop_rows
    P = mc.problem(7, 5, filled="full", seed=9)
    K, N, V = P.K, P.N, P.V
    clean = (P.W.cuda(), P.indptr.cuda(), P.indices.cuda(), P.data.cuda(), P.col.reshape(-1).cuda(), P.val.reshape(-1).cuda(), P.filled.cuda(), K)
    batch = torch.tensor([0, 1, 2, 3, 4, 5], dtype=torch.int32)
    ref = mag_prop_rows(*clean, batch.cuda(), training=False)
    # node 5's bag gets the ids -1 and V; row 2 gets the columns -1 and N; the batch names the rows -1 and S_rows
    hub = 5
    ix = P.indices.clone()
    lo = int(P.indptr[hub])
    ix[lo + 1], ix[lo + 70] = -1, V
    col = P.col.clone()
    col[2, 1], col[2, 2] = -1, N
    bad_batch = torch.tensor([0, 1, -1, 2, 3, P.S_rows, 4, 5], dtype=torch.int32)
    bad = (clean[0], clean[1], ix.cuda(), clean[3], col.reshape(-1).cuda(), clean[5], clean[6], K)
    W = P.W.cuda().requires_grad_(True)
    out = mag_prop_rows(W, *bad[1:], bad_batch.cuda(), training=False)
    assert bool(torch.isfinite(out).all())
    assert not bool(out[2].any()) and not bool(out[5].any())                       # the rows that are not there
    where = {0: 0, 1: 1, 3: 2, 4: 3, 6: 4, 7: 5}                                   # position in bad_batch -> row
    touched = {r for r in range(P.S_rows) if r == 2 or bool((col[r] == hub).any())}
    assert 0 < len(touched) < P.S_rows
    for b, r in where.items():
        if r not in touched:
            assert _same(out[b], ref[r]), (b, r)
    assert not _same(out[3], ref[2])
    n_hub_slots = sum(int((col[r] == hub).sum()) for r in range(P.S_rows))
    want = 2 + 2 + 2 * n_hub_slots                                                 # batch rows + columns + ids, per occurrence
    with pytest.raises(IndexError, match=rf"\b{want} batch row"):
        mag_prop_rows(*bad, bad_batch.cuda(), training=False, validate=True)
    assert mag_prop_rows(*clean, batch.cuda(), training=False, validate=True).shape == ref.shape
    out.sum().backward()                                                           # the backward skips them too
    assert bool(torch.isfinite(W.grad).all()) and bool(W.grad.any())


def test_more_batch_rows_than_the_grid_cap():
    """The launch caps its grid at 8 192 workgroups: a batch above it goes round the grid-stride loop."""
    from grand_plus_amd import mag_prop_rows
    P = mc.problem(1, 1, filled="full", seed=2)
    args = P.cuda()
    B = 8192 + 3
    batch = (torch.arange(B) % P.S_rows).to(torch.int32).cuda()
    small = mag_prop_rows(*args, training=False)
    big = mag_prop_rows(*args, batch, training=False)
    assert big.shape == (B, 1) and _same(big, small[batch.long()])


# ------------------------------------------------------------------------------------- parity with the composed path
def _assert_grad(got, ref, name):
    assert got is not None, name
    scale = float(ref.abs().max())
    torch.testing.assert_close(got.double().cpu(), ref.cpu(), rtol=1e-4, atol=1e-4 * scale + 1e-9, msg=name)   # tests/test_gpu_mlp.py's rule


def test_mag_shaped_step_matches_the_composed_path_and_float64():
    """B = 40, K = 32, H = 64, V = 5 000, mean bag 20, S = 2, no input dropout: emb_rows beside flatten_rows ->
    emb_csr -> random_prop under the same DropNode decisions, each within the rule of the float64 reference; then both
    steps go on through MagMLP, grand_plus_loss(kind="l2") and ClipAdam.step()."""
    from grand_plus_amd import ClipAdam
    from grand_plus_amd.augment import random_prop
    from grand_plus_amd.embedding import flatten_rows
    from grand_plus_amd.mlp import MagMLP
    from grand_plus_amd.objective import grand_plus_loss
    from grand_plus_amd.rows import RowMatrix
    from oracle.mlp_ref import RefMagMLP
    from oracle.objective_ref import grand_loss_ref
    B, K, H, V, C, S, p_node, S_rows, N = 40, 32, 64, 5000, 8, 2, 0.5, 60, 3000
    rng = np.random.default_rng(12)
    lens = rng.integers(1, 40, N)                                                  # mean 20
    indptr = np.zeros(N + 1, np.int64)
    np.cumsum(lens, out=indptr[1:])
    g = torch.Generator().manual_seed(12)
    nnz = int(indptr[-1])
    P = mc.Problem(W=None, indptr=torch.from_numpy(indptr), indices=torch.randint(0, V, (nnz,), generator=g, dtype=torch.int32),
                   data=torch.rand((nnz,), generator=g) + 0.05, col=torch.randint(0, N, (S_rows, K), generator=g, dtype=torch.int32),
                   val=torch.rand((S_rows, K), generator=g, dtype=torch.float64) ** 3 + 1e-9,
                   filled=torch.randint(1, K + 1, (S_rows,), generator=g, dtype=torch.int32), K=K, N=N, V=V, H=H, S_rows=S_rows)
    roundings = K + 39 + S + 8
    assert roundings <= mc.ROUNDINGS
    batch = torch.from_numpy(rng.choice(S_rows, B, replace=False).astype(np.int32))
    keep_rows = (torch.rand((S, S_rows * K), generator=g) >= p_node).to(torch.uint8)
    n_train, tem = 20, 0.5
    labels = torch.randint(0, C, (n_train,), generator=g)
    torch.manual_seed(0)
    fused = MagMLP(V, C, H, 2, True, 0.0, 0.2, True)
    composed = MagMLP(V, C, H, 2, True, 0.0, 0.2, True)
    ref = RefMagMLP(V, C, H, 2, True, 0.0, 0.2, True)
    composed.load_state_dict(fused.state_dict())
    ref.load_state_dict(fused.state_dict())
    fused.cuda().train(); composed.cuda().train(); ref.double().train()
    keeps = [(torch.rand((S, B, fc.weight.shape[1]), generator=g) >= 0.2).to(torch.uint8) for fc in fused.fcs]
    ip, ix, dt = P.indptr.cuda(), P.indices.cuda(), P.data.cuda()
    rm = RowMatrix(np.arange(S_rows), K, None, P.col.reshape(-1).cuda(), P.val.reshape(-1).cuda(), P.filled.cuda(), N)

    # the float64 step
    aug64 = mc.chain64(P, ref.embeds.weight, batch, S, p_node, 0.0, True, keep_rows, 0)
    with torch.no_grad():
        terms = mc.chain64(P, ref.embeds.weight.detach().abs(), batch, S, p_node, 0.0, True, keep_rows, 0)
    z64 = torch.stack([ref(aug64[s], [k[s] for k in keeps]) for s in range(S)])
    loss64 = grand_loss_ref(z64, labels, n_train, 1.0, tem, 0.0, "l2")[0]
    loss64.backward()

    # the fused step, with host synchronisation an error
    opt_f = ClipAdam(fused.parameters(), lr=1e-2, clip_norm=1.0)
    opt_c = ClipAdam(composed.parameters(), lr=1e-2, clip_norm=1.0)
    kc = [k.cuda() for k in keeps]
    y = labels.cuda()
    rows_gpu, keep_gpu = batch.cuda(), keep_rows.cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        aug_f = fused.emb_rows(ip, ix, dt, rm, rows_gpu, samples=S, dropnode_rate=p_node, keep=keep_gpu)
        loss_f, _ = grand_plus_loss(fused(aug_f, keep=kc), y, n_train, 1.0, tem=tem, conf=0.0, kind="l2")
        loss_f.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")

    # the composed step: the same DropNode decisions, gathered into flatten_rows' order
    nbr, scores, mat_idx = flatten_rows(rm.col, rm.val, rm.filled, K, rows_gpu)
    live = torch.arange(K)[None, :] < P.filled.long()[batch.long()][:, None]
    e = (batch.long()[:, None] * K + torch.arange(K)[None, :])[live]
    keep_coo = keep_rows[:, e].contiguous().cuda()
    emb = composed.emb_csr(ip, ix, dt, nodes=nbr)
    aug_c = random_prop(emb, scores, mat_idx, p_node, training=True, keep=keep_coo, samples=S, n_out=B)
    loss_c, _ = grand_plus_loss(composed(aug_c, keep=kc), y, n_train, 1.0, tem=tem, conf=0.0, kind="l2")
    loss_c.backward()

    r_f = mc.close(aug_f.detach(), aug64.detach(), terms, roundings, "fused aug")
    r_c = mc.close(aug_c.detach(), aug64.detach(), terms, roundings, "composed aug")
    print(f"[mag] MAG-shaped step: aug error / bound fused {r_f:.3g}, composed {r_c:.3g}; "
          f"loss fused {loss_f.item():.6f} composed {loss_c.item():.6f} float64 {loss64.item():.6f}")
    for loss in (loss_f, loss_c):
        assert abs(loss.item() - loss64.item()) <= 1e-4 * abs(loss64.item()) + 1e-6
    for model in (fused, composed):
        for (name, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
            _assert_grad(p.grad, q.grad, name)
    assert float(fused.embeds.weight.grad.abs().max()) > 0
    before = [p.detach().clone() for p in fused.parameters()]
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt_f.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    opt_c.step()
    for p0, pf, pc in zip(before, fused.parameters(), composed.parameters()):
        assert bool(torch.isfinite(pf).all()) and not torch.equal(p0, pf)
        assert float((pf.detach() - pc.detach()).abs().max()) <= 2e-2 + 1e-6                        # Adam's first step moves an element by at most lr


def test_forward_and_backward_do_not_synchronise_and_flatten_rows_does():
    from grand_plus_amd import mag_prop_rows
    from grand_plus_amd.embedding import flatten_rows
    c = mc.case("h64_k32_s2")
    _, ip, ix, dt, col, val, filled, K = c["P"].cuda()
    W = c["P"].W.cuda().requires_grad_(True)
    G, batch = c["G"].cuda(), c["batch"].cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = mag_prop_rows(W, ip, ix, dt, col, val, filled, K, batch, **c["kw"])
        (out * G).sum().backward()
        with pytest.raises(RuntimeError):
            flatten_rows(col, val, filled, K, batch)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(W.grad.any())


# -------------------------------------------------------------------------------------------------- deterministic flag
def test_deterministic_with_a_gradient_raises_and_without_one_runs():
    c = mc.case("h7_k5_s3")
    W = c["P"].W.cuda().requires_grad_(True)
    with pytest.raises(RuntimeError, match="deterministic=True"):
        _run(c, W=W, deterministic=True)
    torch.use_deterministic_algorithms(True)
    try:
        with pytest.raises(RuntimeError, match="embedding_bag_csr"):
            _run(c, W=W)
        with torch.no_grad():
            quiet = _run(c, W=W)
    finally:
        torch.use_deterministic_algorithms(False)
    assert _same(quiet, _run(c, deterministic=True)) and _same(quiet, _run(c, deterministic=False))
    assert _run(c, W=W, deterministic=False).requires_grad


# ------------------------------------------------------------------------------------------------------------ valid_mag
@pytest.fixture(scope="module")
def valid_world():
    from grand_plus_amd.rows import RowMatrix
    w, ours, r64 = mc.valid_reference()
    rm = RowMatrix(w["seeds"], mc.MAG_K, None, w["col"].reshape(-1).cuda(), w["val"].reshape(-1).cuda(), w["filled"].cuda(), w["n"])
    return w, ours.cuda(), r64, rm, tuple(t.cuda() for t in w["attrs"])


def _hand_written_valid(model, rm, attrs, idx, y, batch_size):
    """valid_mag's loop from the same ops: (loss, acc, buffers, logits)."""
    from grand_plus_amd import eval_head, eval_reduce, mag_prop_rows
    from grand_plus_amd.evaluate import eval_buffers
    pos = rm.batch_positions(idx, check=True)
    idx = idx.cuda()
    buf = eval_buffers(idx.numel(), idx.device)
    model.eval()
    logits = []
    with torch.no_grad():
        for s in range(0, idx.numel(), batch_size):
            aug = mag_prop_rows(model.embeds.weight, *attrs, rm.col, rm.val, rm.filled, rm.K, pos[s:s + batch_size], training=False)
            logits.append(model(aug))
            eval_head(logits[-1], y, label_rows=idx[s:s + batch_size], out=buf, offset=s)
        loss, acc, _ = eval_reduce(buf)
    return loss, acc, buf, torch.cat(logits)


@pytest.mark.parametrize("batch_size", [1, 7, 200, 203])
def test_valid_mag_equals_the_hand_written_loop_bit_for_bit(valid_world, batch_size):
    from grand_plus_amd import valid_mag
    w, model, _r64, rm, attrs = valid_world
    assert w["idx_val"].numel() == 200
    y = w["y"].cuda()
    loss0, acc0, buf0, _ = _hand_written_valid(model, rm, attrs, w["idx_val"], y, batch_size)
    for training in (True, False):
        model.train(training)
        loss, acc, counts = valid_mag(model, rm, *attrs, w["idx_val"], y, batch_size=batch_size, return_counts=True)
        assert model.training is training and torch.cuda.get_sync_debug_mode() == 0 and torch.is_grad_enabled()
        assert loss.is_cuda and loss.dim() == 0 and _same(loss, loss0) and _same(acc, acc0)
    n_correct = int((buf0.pred.cpu().long() == w["y"][w["idx_val"]]).sum())
    assert counts.tolist() == [200, n_correct, 0, 0]


def test_valid_mag_against_the_float64_chain(valid_world):
    """Loss: assert_loss's rule, with plain torch in float32 (index_add_ embedding and propagation, the restatement of
    the MLP in float32) as its yardstick, and evaluate_cases.chain64's derived bound.  Predictions: every decided row."""
    import torch.nn.functional as Fn
    from grand_plus_amd import valid_mag
    from oracle.mlp_ref import RefMagMLP
    from augment_cases import rows_to_coo
    w, model, r64, rm, attrs = valid_world
    y = w["y"].cuda()
    loss, acc, counts = valid_mag(model, rm, *attrs, w["idx_val"], y, batch_size=64, return_counts=True)
    _, _, buf, _ = _hand_written_valid(model, rm, attrs, w["idx_val"], y, 64)
    # plain torch, float32, on the GPU
    ip, ix, dt = attrs
    n = w["n"]
    W = model.embeds.weight.detach()
    node = torch.repeat_interleave(torch.arange(n, device="cuda"), ip[1:] - ip[:-1])
    emb = torch.zeros((n, mc.MAG_H), device="cuda").index_add_(0, node, W[ix.long()] * dt[:, None]) / \
        (torch.zeros((n, 1), device="cuda").index_add_(0, node, dt[:, None]) + 1e-10)
    pos = torch.from_numpy(np.searchsorted(w["seeds"], w["idx_val"].numpy()))
    idx, cols, scores, _ = rows_to_coo(w["col"], w["val"], w["filled"], mc.MAG_K, pos)
    idx, cols, scores = idx.cuda(), cols.cuda(), scores.cuda()
    aug = torch.zeros((pos.numel(), mc.MAG_H), device="cuda").index_add_(0, idx, emb[cols] * scores[:, None]) / \
        (torch.zeros((pos.numel(), 1), device="cuda").index_add_(0, idx, scores[:, None]) + 1e-12)
    plain = RefMagMLP(mc.MAG_V, mc.MAG_C, mc.MAG_H, 2, True, 0.0, 0.5, True)
    plain.load_state_dict(model.state_dict())
    plain.cuda().eval()
    with torch.no_grad():
        torch32 = float(Fn.nll_loss(Fn.log_softmax(plain(aug, None), dim=-1), y[w["idx_val"].cuda()]))
    ec.assert_loss(float(loss), torch32, r64["loss"], "valid_mag")
    print(f"[mag] valid_mag: |loss-loss64| {abs(float(loss) - r64['loss']):.3e}, derived bound {r64['loss_bound']:.3e}")
    assert abs(float(loss) - r64["loss"]) <= r64["loss_bound"]
    ec.assert_decided_preds(buf.pred, r64, "valid_mag")
    n_correct = int((buf.pred.cpu().long() == w["y"][w["idx_val"]]).sum())
    assert counts.tolist() == [200, n_correct, 0, 0] and float(acc) == float(np.float32(n_correct / 200))


def test_valid_mag_raises_for_a_node_that_is_no_seed(valid_world):
    from grand_plus_amd import valid_mag
    w, model, _r64, rm, attrs = valid_world
    seeds = set(w["seeds"].tolist())
    stranger = next(i for i in range(w["n"]) if i not in seeds)
    model.train()
    with pytest.raises(KeyError):
        valid_mag(model, rm, *attrs, [int(w["idx_val"][0]), stranger], w["y"].cuda())
    assert model.training and torch.cuda.get_sync_debug_mode() == 0


# ---------------------------------------------------------------------------------------------------------- predict_mag
@pytest.fixture(scope="module")
def predict_world():
    from grand_plus_amd import Graph, synth
    indptr, indices = synth.shape_csr("tiny")
    n = len(indptr) - 1
    ours, _ = mc.mag_model_pair()
    rng = np.random.default_rng(8)
    idx = rng.permutation(n)[:300].astype(np.int64)
    idx[5] = idx[200]
    y = torch.from_numpy(rng.integers(0, mc.MAG_C, n)).cuda()
    return Graph(indptr, indices, 0), tuple(t.cuda() for t in mc.mag_attributes(n)), ours.cuda(), idx, y


@pytest.mark.parametrize("infer", [False, True])
@pytest.mark.parametrize("mode", ["ppr", "avg", "single"])
def test_predict_mag_equals_predict_on_the_precomputed_embedding(predict_world, mode, infer):
    from grand_plus_amd import predict, predict_mag
    from grand_plus_amd.embedding import embedding_bag_csr
    graph, attrs, model, idx, y = predict_world
    model.train()
    acc, preds = predict_mag(graph, *attrs, model, idx, y, mode, 2, alpha=0.2, return_preds=True, infer=infer)
    assert model.training and torch.cuda.get_sync_debug_mode() == 0 and torch.is_grad_enabled()
    with torch.no_grad():
        emb = embedding_bag_csr(model.embeds.weight, *attrs, nodes=None, training=False, validate=False)
    acc0, preds0 = predict(graph, emb, model, idx, y, mode, 2, alpha=0.2, return_preds=True, infer=infer)
    assert acc.is_cuda and acc.dim() == 0 and _same(acc, acc0) and torch.equal(preds, preds0)
    assert preds.shape == (300,) and len(set(preds.tolist())) > 1
