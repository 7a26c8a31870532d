"""The eval-only MLP forward: `infer`, `local_logits` and `predict(infer=True)` on the GPU.  Where the block
path of §7f takes one k-chain per output the two must agree bit for bit (k-order, prologue, row scale, BatchNorm fold);
everywhere the outputs follow tests/test_gpu_mlp.py's rule against the float64 restatement (tests/infer_cases.py)."""
import numpy as np
import pytest
import torch

import infer_cases as ic

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _block(model, X):
    """The block path in eval mode, without grad: what infer is held to."""
    was = model.training
    model.eval()
    with torch.no_grad():
        out = model(X)
    model.train(was)
    return out


@pytest.fixture(scope="module")
def chunk_model():
    ours, ref = ic.pair(ic.CHUNK)
    X = ic.inputs(ic.CHUNK, 385).cuda()
    ours = ours.cuda()
    return ours, X, ours.infer(X)


# ------------------------------------------------------------------------------------ 1. bitwise against the block path
@pytest.mark.parametrize("B", ic.BITWISE_ROWS)
@pytest.mark.parametrize("case", ic.BITWISE, ids=[c[0] for c in ic.BITWISE])
def test_infer_equals_the_block_path_bit_for_bit_where_it_takes_one_chain(case, B):
    ours, _ = ic.pair(case)
    ours = ours.cuda()
    X = ic.inputs(case, B).cuda()
    got = ours.infer(X)
    assert got.shape == (B, case[4]) and got.dtype == torch.float32
    assert _same(got, _block(ours, X))


def test_infer_equals_the_block_path_at_128_tiles_and_k_200():
    ours, _ = ic.pair(ic.TILE_COUNT)
    ours = ours.cuda()
    X = ic.inputs(ic.TILE_COUNT, 4096).cuda()
    assert _same(ours.infer(X), _block(ours, X))


# ------------------------------------------------------------------------------------------------- 2. against float64
@pytest.mark.parametrize("B", ic.CASE_ROWS)
@pytest.mark.parametrize("case", ic.CASES, ids=[c[0] for c in ic.CASES])
def test_infer_matches_the_float64_restatement(case, B):
    ours, ref = ic.pair(case)
    X = ic.inputs(case, B).cuda()
    got = ours.cuda().infer(X)
    want, bound = ic.ref_out(ref.cuda(), X.double())
    ic.assert_rule(got, want, bound, f"{case[0]} B={B}")


@pytest.mark.parametrize("case,B", ic.SMALL_DRAWN, ids=[c[0] for c, _ in ic.SMALL_DRAWN])
def test_infer_at_small_running_variances_and_one_epsilon_per_layer(case, B):
    """Running variances from 0 to 1e-3, bn.eps = 1e-3, 1e-5, 1e-7 by layer and a row whose norm is node_norm's 1e-12: here
    the epsilons decide the logits (tests/test_host_mutants.py), under the same rule."""
    ours, ref = ic.small_pair(case)
    X = ic.small_inputs(case, B).cuda()
    ours = ours.cuda()
    got = ours.infer(X)
    want, bound = ic.ref_out(ref.cuda(), X.double())
    ic.assert_rule(got, want, bound, f"{case[0]} small_var B={B}")
    if case in ic.SMALL_VAR_BITWISE:
        assert _same(got, _block(ours, X))


# ------------------------------------------------------------------------------------- 3. tile and reduction edges
@pytest.mark.parametrize("f_in,f_out", ic.EDGE_SHAPES)
def test_tile_and_reduction_edges(f_in, f_out):
    B = ic.EDGE_ROWS
    m = ic.single_layer(f_in, f_out).cuda()
    X = torch.randn((B, f_in), generator=torch.Generator().manual_seed(f_in * 7 + f_out)).cuda()
    got = m.infer(X)
    fc = m.fcs[0]
    X64, W64, b64 = X.double(), fc.weight.detach().double(), fc.bias.detach().double()
    want = X64 @ W64.t() + b64
    bound = 2e-5 * (X64.abs() @ W64.abs().t() + b64.abs()) + 1e-6
    ic.assert_rule(got, want, bound, f"{f_in}->{f_out}")
    if f_in <= 64:
        assert _same(got, _block(m, X))


# ------------------------------------------------------------------------- 4. row independence and chunking, bitwise
@pytest.mark.parametrize("b", [1, 100, 128, 384, 385, 1000])
def test_any_batch_size_gives_the_same_bits(chunk_model, b):
    ours, X, whole = chunk_model
    assert _same(ours.infer(X, batch_size=b), whole)


@pytest.mark.parametrize("i,j", [(0, 1), (127, 129), (128, 256), (384, 385)])
def test_a_row_slice_gives_the_rows_of_the_whole(chunk_model, i, j):
    ours, X, whole = chunk_model
    assert _same(ours.infer(X[i:j].contiguous()), whole[i:j])


def test_a_nan_row_stays_in_its_row(chunk_model):
    ours, X, whole = chunk_model
    Xn = X.clone()
    Xn[5] = float("nan")
    got = ours.infer(Xn)
    assert bool(torch.isnan(got[5]).all())
    keep = torch.arange(385, device="cuda") != 5
    assert _same(got[keep], whole[keep])


# ------------------------------------------------------------------------------------------------------ 5. alignment
@pytest.mark.parametrize("F", [7, 6, 100])
def test_a_row_slice_at_any_alignment_equals_its_copy(F):
    case = ("align", "model", F, 33, 5, 2, True, True)
    ours, _ = ic.pair(case)
    ours = ours.cuda()
    base = torch.randn((301, F), generator=torch.Generator().manual_seed(F)).cuda()
    view = base[1:]                                          # 4 F bytes past the allocation: 28, 24 and 400
    assert view.is_contiguous() and view.data_ptr() == base.data_ptr() + 4 * F
    assert _same(ours.infer(view), ours.infer(view.clone()))


def test_the_scalar_load_path_equals_the_vector_path():
    """F = 100 at a pointer that is only 4-byte aligned takes scalar loads; its copy takes 16-byte loads."""
    case = ("align100", "model", 100, 130, 47, 2, True, True)
    ours, _ = ic.pair(case)
    ours = ours.cuda()
    flat = torch.randn(1 + 300 * 100, generator=torch.Generator().manual_seed(3)).cuda()
    view = flat[1:].view(300, 100)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    assert _same(ours.infer(view), ours.infer(view.clone()))


# ------------------------------------------------------------------------------------------------------ 6. many rows
def test_seventy_thousand_rows():
    case = ("rows70k", "model", 100, 64, 47, 2, True, True)
    ours, ref = ic.pair(case)
    ours = ours.cuda()
    B = 70001
    X = torch.randn((B, 100), generator=torch.Generator().manual_seed(11)).cuda()
    got = ours.infer(X)
    sub = torch.randperm(B, generator=torch.Generator().manual_seed(12))[:2000].cuda()
    want, bound = ic.ref_out(ref.cuda(), X[sub].double())
    ic.assert_rule(got[sub], want, bound, "70 001 rows")
    assert _same(ours.infer(X, batch_size=10000), got)


def test_more_than_65535_row_tiles_exactly():
    """128 * 65 535 + 37 rows of (2 -> 1): small integers, so the chain x0 w0, then fma(x1, w1, .), then + b is exact."""
    B = 128 * 65535 + 37
    m = ic.single_layer(2, 1).cuda()
    with torch.no_grad():
        m.fcs[0].weight.copy_(torch.tensor([[3.0, -5.0]]))
        m.fcs[0].bias.copy_(torch.tensor([7.0]))
    X = torch.randint(-8, 9, (B, 2), device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)).float()
    got = m.infer(X)
    X64 = X.double()
    want = (torch.addcmul(X64[:, 0] * 3.0, X64[:, 1], torch.tensor(-5.0, dtype=torch.float64, device="cuda")) + 7.0).float()
    assert got.shape == (B, 1) and torch.equal(got[:, 0], want)


# -------------------------------------------------------------------------------------------- 7. module state and API
def test_infer_leaves_the_module_alone_and_never_synchronises():
    ours, _ = ic.pair(ic.CHUNK)
    ours = ours.cuda()
    X = ic.inputs(ic.CHUNK, 257).cuda().requires_grad_(True)
    state = {k: v.clone() for k, v in ours.state_dict().items()}
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ours.train()
        in_train = ours.infer(X)
        assert ours.training
        ours.eval()
        in_eval = ours.infer(X)
        assert not ours.training
        out = torch.empty((257, 5), device="cuda")
        ret = ours.infer(X, out=out, batch_size=100)
        empty = ours.infer(X[:0])
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.is_grad_enabled()
    assert not in_train.requires_grad and in_train.grad_fn is None
    assert _same(in_train, in_eval)
    assert ret is out and _same(out, in_eval)
    assert empty.shape == (0, 5) and empty.dtype == torch.float32 and empty.is_cuda
    after = ours.state_dict()
    assert set(after) == set(state)
    for k, v in state.items():                               # running statistics and num_batches_tracked included
        assert torch.equal(after[k], v), k


def test_a_mag_model_without_layers_returns_its_input():
    from grand_plus_amd.mlp import MagMLP
    m = MagMLP(10, 4, 16, 1, False, 0.0, 0.0, False).cuda()
    X = torch.randn((9, 4), device="cuda")
    assert m.infer(X) is X
    out = torch.empty_like(X)
    assert m.infer(X, out=out) is out and torch.equal(out, X)


# ---------------------------------------------------------------------------- 8. local_logits and predict(infer=True)
@pytest.fixture(scope="module")
def graph():
    from grand_plus_amd import Graph
    indptr, indices = ic.graph_csr()
    return Graph(indptr, indices, 0)


@pytest.mark.parametrize("batch", [10000, 70000])
@pytest.mark.parametrize("mode", ["ppr", "avg", "single"])
def test_predict_with_infer_equals_the_batch_loop(graph, mode, batch):
    from grand_plus_amd import predict
    ours, _ = ic.pair(ic.SMALL)
    ours = ours.cuda().train()
    X, y, idx = ic.graph_features(ic.SMALL[2]).cuda(), ic.graph_labels(ic.SMALL[4]).cuda(), ic.query_ids()
    acc0, preds0 = predict(graph, X, ours, idx, y, mode, 2, batch_size_logits=batch, return_preds=True)
    acc1, preds1 = predict(graph, X, ours, idx, y, mode, 2, batch_size_logits=batch, return_preds=True, infer=True)
    assert ours.training and torch.cuda.get_sync_debug_mode() == 0 and torch.is_grad_enabled()
    assert torch.equal(preds1, preds0) and _same(acc1.reshape(1), acc0.reshape(1))
    assert len(set(preds1.tolist())) > 1                     # not one class for every row


def test_predict_with_infer_on_the_reddit_shape_follows_the_float64_chain(graph):
    from grand_plus_amd import local_logits, predict
    ours, _ = ic.reddit_pair()
    ours = ours.cuda()
    X, y = ic.graph_features(ic.REDDIT[2]).cuda(), ic.graph_labels(ic.REDDIT[4]).cuda()
    idx = torch.arange(ic.N_NODES)
    acc, preds = predict(graph, X, ours, idx, y, "ppr", 2, alpha=0.2, return_preds=True, infer=True)
    z = local_logits(ours, graph.propagate_features(X, "ppr", 2, 0.2))
    assert z.shape == (ic.N_NODES, 41) and not z.requires_grad
    own = torch.argmax(z, dim=1)
    assert torch.equal(preds.long(), own)
    assert float(acc) == float(np.float32(int((own == y).sum()) / ic.N_NODES))
    out = torch.empty_like(z)
    assert local_logits(ours, graph.propagate_features(X, "ppr", 2, 0.2), batch_size=3000, out=out) is out and _same(out, z)
    pred64, decided = ic.reddit_chain64("ppr", 2, 0.2)
    left_out = 1.0 - float(decided.double().mean())
    print(f"[infer] reddit shape: {left_out:.5f} of the rows within the margin")
    assert left_out <= ic.LEFT_OUT
    assert torch.equal(preds.cpu().long()[decided], pred64[decided])
