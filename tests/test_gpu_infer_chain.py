"""`infer(fused=True)` on the GPU: the last two blocks as one kernel, the hidden tile in LDS.  The contract is
the bits of the unfused `infer` for every shape, flag set, alignment and number of rows; two shapes are also held to the
float64 restatement, in case both paths share a fault."""
import functools

import pytest
import torch

import infer_cases as ic
import infer_chain_cases as cc

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _model(case):
    return cc.model(case).cuda()


def _assert_fused_equals_unfused(case, B, seed=7):
    m = _model(case)
    X = ic.inputs(case, B, seed).cuda()
    want = m.infer(X)
    got = m.infer(X, fused=True)
    assert got.shape == (B, case[4]) and got.dtype == torch.float32
    assert bool(torch.isfinite(want).all())
    assert _same(got, want), f"{case[0]} B={B}: {int((_bits(got) != _bits(want)).sum())} outputs differ"
    return got


# ----------------------------------------------------------------------------------- 1. bitwise against unfused infer
@pytest.mark.parametrize("B", cc.ROWS)
@pytest.mark.parametrize("case", cc.CASES, ids=[c[0] for c in cc.CASES])
def test_fused_equals_unfused_bit_for_bit(case, B):
    _assert_fused_equals_unfused(case, B)


@pytest.mark.parametrize("case", cc.ONE_BLOCK, ids=[c[0] for c in cc.ONE_BLOCK])
def test_a_one_block_model_is_refused_on_the_gpu_too(case):
    m = _model(case)
    with pytest.raises(ValueError, match="fewer than two blocks"):
        m.infer(ic.inputs(case, 33).cuda(), fused=True)


# ------------------------------------------------------------------------------------------------------- 2. flag sets
@pytest.mark.parametrize("use_bn,node_norm", cc.FLAG_SETS)
@pytest.mark.parametrize("shape", cc.FLAG_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_every_flag_set(shape, use_bn, node_norm):
    _assert_fused_equals_unfused(cc.two_block(*shape, use_bn, node_norm), cc.B)


# ------------------------------------------------------------------------------------------ 3. hidden and class edges
@pytest.mark.parametrize("C", cc.CLASS_EDGES)
@pytest.mark.parametrize("H", cc.HIDDEN_EDGES)
def test_hidden_and_class_edges(H, C):
    _assert_fused_equals_unfused(cc.two_block(cc.EDGE_F_IN, H, C), cc.B)


# --------------------------------------------------------------------------------------- 4. reduction edges of block 1
@pytest.mark.parametrize("f_in", cc.K_EDGES)
def test_reduction_edges_of_the_first_block(f_in):
    _assert_fused_equals_unfused(cc.two_block(f_in, 130, 5), cc.B)


# ---------------------------------------------------------------------------------------------------- 5. float64 rule
@pytest.mark.parametrize("name", cc.RULE_CASES)
def test_fused_matches_the_float64_restatement(name):
    case = next(c for c in ic.CASES if c[0] == name)
    ours, ref = ic.pair(case)
    X = ic.inputs(case, cc.RULE_ROWS).cuda()
    got = ours.cuda().infer(X, fused=True)
    want, bound = ic.ref_out(ref.cuda(), X.double())
    ic.assert_rule(got, want, bound, f"fused {name} B={cc.RULE_ROWS}")


@pytest.mark.parametrize("case,B", ic.SMALL_DRAWN, ids=[c[0] for c, _ in ic.SMALL_DRAWN])
def test_fused_at_small_running_variances_and_one_epsilon_per_layer(case, B):
    """The two fused blocks take their own epsilons (bn1_eps, bn2_eps): unequal ones at variances they decide."""
    ours, ref = ic.small_pair(case)
    X = ic.small_inputs(case, B).cuda()
    ours = ours.cuda()
    got = ours.infer(X, fused=True)
    assert _same(got, ours.infer(X))
    want, bound = ic.ref_out(ref.cuda(), X.double())
    ic.assert_rule(got, want, bound, f"fused {case[0]} small_var B={B}")


# ------------------------------------------------------------------------------------------------------------ 6. rows
@pytest.fixture(scope="module")
def chunk():
    m = _model(cc.CHUNK)
    X = ic.inputs(cc.CHUNK, cc.CHUNK_ROWS).cuda()
    return m, X, m.infer(X)


@pytest.mark.parametrize("b", [1, 7, 32, 100, cc.CHUNK_ROWS, cc.CHUNK_ROWS + 3])
def test_any_batch_size_gives_the_same_bits(chunk, b):
    m, X, whole = chunk
    assert _same(m.infer(X, batch_size=b, fused=True), whole)


@pytest.mark.parametrize("F", [7, 6, 100])
def test_a_row_slice_at_any_alignment_equals_its_copy(F):
    m = _model(cc.two_block(F, 33, 5))
    base = torch.randn((301, F), generator=torch.Generator().manual_seed(F)).cuda()
    view = base[1:]                                          # 4 F bytes past the allocation: 28, 24 and 400
    assert view.is_contiguous() and view.data_ptr() == base.data_ptr() + 4 * F
    got = m.infer(view, fused=True)
    assert _same(got, m.infer(view.clone(), fused=True)) and _same(got, m.infer(view.clone()))


def test_the_scalar_load_path_equals_the_vector_path():
    """F = 100 at a pointer that is only 4-byte aligned takes scalar loads; its copy takes 16-byte loads."""
    m = _model(cc.two_block(100, 132, 47))
    flat = torch.randn(1 + 300 * 100, generator=torch.Generator().manual_seed(3)).cuda()
    view = flat[1:].view(300, 100)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    got = m.infer(view, fused=True)
    assert _same(got, m.infer(view.clone(), fused=True)) and _same(got, m.infer(view.clone()))


# ------------------------------------------------------------------------------------------------- 7. NaN containment
@pytest.mark.parametrize("case", [cc.CHUNK, cc.two_block(100, 1024, 47)], ids=["three_blocks", "amazon_shape"])
def test_a_nan_row_stays_in_its_row(case):
    m = _model(case)
    B = 131
    X = ic.inputs(case, B).cuda()
    whole = m.infer(X)
    Xn = X.clone()
    Xn[37, 3] = float("nan")
    got = m.infer(Xn, fused=True)
    assert bool(torch.isnan(got[37]).all())
    keep = torch.arange(B, device="cuda") != 37
    assert _same(got[keep], whole[keep])


# ------------------------------------------------------------------------------------------------- 8. large row count
def test_seventy_thousand_rows():
    _assert_fused_equals_unfused(cc.MAG_LARGE, cc.LARGE_ROWS)


# ------------------------------------------------------------------------------ 9. the hidden layer is not materialised
def test_the_hidden_tensor_is_never_allocated():
    case, B = cc.AMAZON, cc.MEMORY_ROWS
    H = case[3]
    m = _model(case)
    X = ic.inputs(case, B).cuda()
    bound = 4 * B * H // 2                                   # half the [B, H] float32 tensor

    def peak(**kw):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = m.infer(X, **kw)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, out

    fused_peak, got = peak(fused=True)
    unfused_peak, want = peak()
    print(f"[infer chain] peak allocation above the start: fused {fused_peak} B, unfused {unfused_peak} B, bound {bound} B")
    assert unfused_peak > bound                              # the measure sees the hidden tensor
    assert fused_peak < bound
    assert _same(got, want)


# ------------------------------------------------------------------------------------------------- 10. module state
def test_fused_infer_leaves_the_module_alone_and_never_synchronises():
    m = cc.model(cc.CHUNK).cuda()
    X = ic.inputs(cc.CHUNK, 257).cuda().requires_grad_(True)
    want = m.infer(X)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        m.train()
        in_train = m.infer(X, fused=True)
        assert m.training
        m.eval()
        in_eval = m.infer(X, fused=True)
        assert not m.training
        out = torch.empty((257, 5), device="cuda")
        ret = m.infer(X, out=out, batch_size=100, fused=True)
        empty = m.infer(X[:0], fused=True)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert torch.is_grad_enabled()
    assert not in_train.requires_grad and in_train.grad_fn is None
    assert _same(in_train, want) and _same(in_eval, want)
    assert ret is out and _same(out, want)
    assert empty.shape == (0, 5) and empty.dtype == torch.float32 and empty.is_cuda
    after = m.state_dict()
    assert set(after) == set(state)
    for k, v in state.items():                               # running statistics and num_batches_tracked included
        assert torch.equal(after[k], v), k


# ------------------------------------------------------------------------------------------------------- 11. predict
@pytest.fixture(scope="module")
def graph():
    from grand_plus_amd import Graph
    indptr, indices = ic.graph_csr()
    return Graph(indptr, indices, 0)


@pytest.mark.parametrize("mode", ["ppr", "avg"])
def test_predict_fused_equals_predict_with_infer(graph, mode):
    from grand_plus_amd import local_logits, predict
    ours, _ = ic.pair(ic.SMALL)
    ours = ours.cuda().train()
    X, y, idx = ic.graph_features(ic.SMALL[2]).cuda(), ic.graph_labels(ic.SMALL[4]).cuda(), ic.query_ids()
    acc0, preds0 = predict(graph, X, ours, idx, y, mode, 2, return_preds=True, infer=True)
    acc1, preds1 = predict(graph, X, ours, idx, y, mode, 2, return_preds=True, infer=True, fused=True)
    assert ours.training and torch.cuda.get_sync_debug_mode() == 0 and torch.is_grad_enabled()
    assert torch.equal(preds1, preds0) and _same(acc1.reshape(1), acc0.reshape(1))
    assert len(set(preds1.tolist())) > 1
    prop = graph.propagate_features(X, mode, 2, 0.2)
    assert _same(local_logits(ours, prop, fused=True), local_logits(ours, prop))
