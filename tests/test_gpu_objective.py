"""The fused GRAND+ objective against the float64 restatement of the reference in oracle/objective_ref.py:
log_softmax + F.nll_loss per sample (model.py:323-327) and consis_loss (model.py:123-139), through autograd.
Tolerances: the loss within 1e-5 |ref| + 1e-7; dz per element within 1e-5 max|ref row| + 1e-7.  The edge tests
(upstream gradients, log-prob mode with labels, S up to 16, C from 1 to 4 096, B from 0 to a second grid-stride trip,
sharpening where fp32 pow underflows, argmax ties, strided inputs) draw their cases from objective_cases.py, which
test_host_objective.py proves on the CPU first.  Ends with two training steps end to end: a Cora-shaped one with
BatchNorm and the MAG-shaped one of test_gpu_embedding.py, both with --sample 2."""
import math

import numpy as np
import pytest

import objective_cases as oc
from augment_cases import rows_to_coo
from oracle.objective_ref import consis_loss_ref, grand_loss_ref

pytestmark = pytest.mark.gpu


def _logits(S, B, C, seed, scale=3.0):
    import torch
    g = torch.Generator().manual_seed(seed)
    return torch.randn((S, B, C), generator=g) * scale, g


def _check(z, labels, n_l, w, tem, conf, kind, ref_labels=None, expect_nan=False):
    """Runs both sides; returns (loss, parts, dz) of the kernels."""
    import torch
    from grand_plus_amd.objective import grand_plus_loss
    S, B, C = z.shape
    conf_v = 2.0 / C if conf is None else conf
    z64 = z.double().requires_grad_(True)
    rl = labels if ref_labels is None else ref_labels
    ref, ref_sup, ref_con = grand_loss_ref(z64, rl, n_l, w, tem, conf_v, kind)
    if ref.requires_grad:
        ref.backward()
    zc = z.cuda().requires_grad_(True)
    loss, parts = grand_plus_loss(zc, labels.cuda() if labels is not None else None, n_l, w, tem=tem, conf=conf, kind=kind)
    loss.backward()
    for got, want in ((loss, ref), (parts["sup"], ref_sup), (parts["con"], ref_con)):
        got, want = float(got), float(want)
        if math.isnan(want):
            assert math.isnan(got)
        else:
            assert abs(got - want) <= 1e-5 * abs(want) + 1e-7, (got, want)
    if expect_nan:
        assert math.isnan(float(loss))
    gref = z64.grad if z64.grad is not None else torch.zeros_like(z64)
    dz = zc.grad.double().cpu()
    tol = 1e-5 * gref.abs().amax(dim=-1, keepdim=True) + 1e-7
    bad = (dz - gref).abs() > tol
    assert not bool(bad.any()), f"{int(bad.sum())} gradient elements off; max |d| {float((dz - gref).abs().max()):.3e}"
    avg_p = torch.exp(torch.log_softmax(z.double(), -1)).mean(0)
    assert int(parts["n_conf"]) == int((avg_p[n_l:].max(1)[0] > conf_v).sum())
    return loss, parts, zc.grad


@pytest.mark.parametrize("C", [3, 7, 41, 100, 349])
@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("n_l", [0, 5, 50])
@pytest.mark.parametrize("kind", ["kl", "l2"])
def test_loss_and_gradient_match_the_reference(C, S, n_l, kind):
    import torch
    tem = (0.1, 0.5, 1.0)[(C + S + n_l) % 3]
    B = n_l + 70
    z, g = _logits(S, B, C, seed=C * 31 + S * 7 + n_l + (kind == "kl"), scale=3.0 if C < 100 else 6.0)
    labels = torch.randint(0, C, (max(n_l, 1),), generator=g)
    w = 0.7
    loss, parts, _ = _check(z, labels, n_l, w, tem, None, kind, expect_nan=(n_l == 0))
    if n_l:
        assert int(parts["n_valid"]) == n_l
        pred = z[S - 1, :n_l].argmax(1)
        assert int(parts["n_correct"]) == int((pred == labels[:n_l]).sum())


def test_many_rows_use_several_reduce_partials():
    import torch
    z, g = _logits(2, 10000, 41, seed=5)
    labels = torch.randint(0, 41, (2000,), generator=g)
    _check(z, labels, 2000, 1.0, 0.1, None, "kl")


def test_no_confident_row_gives_nan_and_the_supervised_gradient():
    import torch
    from grand_plus_amd.objective import grand_plus_loss
    z, g = _logits(2, 60, 7, seed=9)
    labels = torch.randint(0, 7, (20,), generator=g)
    loss, parts, dz = _check(z, labels, 20, 1.0, 0.5, 1.0, "l2", expect_nan=True)   # avg_p.max > 1 never holds
    assert int(parts["n_conf"]) == 0 and math.isnan(float(parts["con"]))
    z64 = z.double().requires_grad_(True)
    grand_loss_ref(z64, labels, 20, 1.0, 0.5, 1.0, "l2")[1].backward()           # L_sup alone
    torch.testing.assert_close(dz.double().cpu(), z64.grad, rtol=1e-4, atol=1e-7)
    assert torch.count_nonzero(dz[:, 20:]) == 0


def test_every_row_confident_and_weight_zero():
    import torch
    z, g = _logits(3, 80, 7, seed=10)
    labels = torch.randint(0, 7, (30,), generator=g)
    _, parts, _ = _check(z, labels, 30, 0.5, 0.5, -1.0, "kl")
    assert int(parts["n_conf"]) == 50
    loss, parts, dz = _check(z, labels, 30, 0.0, 0.5, None, "l2")                 # weight 0: the loss is L_sup
    assert float(loss) == pytest.approx(float(parts["sup"]), rel=1e-6)
    assert torch.count_nonzero(dz[:, 30:]) == 0


def test_ignore_index_rows_are_left_out():
    import torch
    z, g = _logits(2, 60, 7, seed=12)
    labels = torch.randint(0, 7, (20,), generator=g)
    labels[1] = -100; labels[7] = -100
    _, parts, dz = _check(z, labels, 20, 1.0, 0.5, None, "kl")
    assert int(parts["n_valid"]) == 18 and int(parts["n_bad_labels"]) == 0
    assert torch.count_nonzero(dz[:, 1]) == 0 and torch.count_nonzero(dz[:, 7]) == 0


def test_out_of_range_labels_are_counted_not_read():
    import torch
    from grand_plus_amd.objective import grand_plus_loss
    z, g = _logits(2, 60, 7, seed=13)
    labels = torch.randint(0, 7, (20,), generator=g)
    labels[0] = 7; labels[4] = -5; labels[9] = 1 << 40
    ref_labels = labels.clone(); ref_labels[[0, 4, 9]] = -100
    _, parts, _ = _check(z, labels, 20, 1.0, 0.5, None, "l2", ref_labels=ref_labels)
    assert int(parts["n_bad_labels"]) == 3 and int(parts["n_valid"]) == 17
    with pytest.raises(IndexError):
        grand_plus_loss(z.cuda(), labels.cuda(), 20, 1.0, tem=0.5, validate=True)
    loss, parts = grand_plus_loss(z.cuda(), labels.clamp(0, 6).cuda(), 20, 1.0, tem=0.5, validate=True)
    assert int(parts["n_bad_labels"]) == 0 and math.isfinite(float(loss))


@pytest.mark.parametrize("kind", ["kl", "l2"])
@pytest.mark.parametrize("tem", [0.1, 0.5, 1.0])
def test_log_prob_mode_is_consis_loss(kind, tem):
    import torch
    from grand_plus_amd.objective import consis_loss
    z, _ = _logits(3, 90, 41, seed=int(tem * 10) + (kind == "kl"))
    lp64 = [torch.log_softmax(z[s].double(), -1).detach().requires_grad_(True) for s in range(3)]
    ref = consis_loss_ref(lp64, tem, 2.0 / 41, kind)
    ref.backward()
    lps = [torch.log_softmax(z[s], -1).cuda().requires_grad_(True) for s in range(3)]
    got = consis_loss(lps, tem, 2.0 / 41, loss=kind)
    got.backward()
    assert abs(float(got) - float(ref)) <= 1e-5 * abs(float(ref)) + 1e-7
    for a, b in zip(lps, lp64):
        tol = 1e-5 * b.grad.abs().amax(dim=-1, keepdim=True) + 1e-7
        assert not bool(((a.grad.double().cpu() - b.grad).abs() > tol).any())


def _run(case, coeffs=(1, 0, 0)):
    """One case of objective_cases.py through the kernels, differentiated as a*loss + b*L_sup + c*L_con (terms with a
    zero coefficient left out, so autograd passes None for them): value, parts and dz against the float64 reference
    under the file's tolerance, the four counts against float64 and torch.argmax.  Returns (loss, parts, dz)."""
    from grand_plus_amd.objective import grand_plus_loss
    z, labels, n_l, conf = oc.build(case)
    ref = oc.reference(case, tuple(coeffs))
    zc = z.cuda().requires_grad_(True)
    loss, parts = grand_plus_loss(zc, labels.cuda(), n_l, case.w, tem=case.tem, conf=conf, kind=case.kind,
                                  inputs_are_log_probs=case.log_probs)
    oc.combine((loss, parts["sup"], parts["con"]), coeffs).backward()
    oc.assert_matches({"loss": loss, "sup": parts["sup"], "con": parts["con"]}, zc.grad, ref, f"{oc.case_id(case)} {tuple(coeffs)}")
    want = oc.counts(case)
    assert {k: int(parts[k]) for k in want} == want
    return loss, parts, zc.grad


@pytest.mark.parametrize("case", oc.UPSTREAM, ids=oc.case_id)
def test_upstream_gradients_of_the_loss_and_both_parts(case):
    """c_sup = (g_loss + g_sup) / (S n_valid), c_con = (w g_loss + g_con) / (S n_conf), each upstream gradient present,
    absent (None) and of either sign; weight positive, 0 and negative."""
    import torch
    for coeffs in oc.COEFFS:
        _, _, dz = _run(case, coeffs)
        assert float(dz.abs().max()) > 0
        if coeffs == (0, 1, 0):
            assert torch.count_nonzero(dz[:, case.n_l:]) == 0 and torch.count_nonzero(dz[:, :case.n_l]) > 0
        if coeffs == (0, 0, 1):
            assert torch.count_nonzero(dz[:, :case.n_l]) == 0 and torch.count_nonzero(dz[:, case.n_l:]) > 0


@pytest.mark.parametrize("case", oc.LOGPROB, ids=oc.case_id)
def test_log_prob_mode_with_labels(case):
    """inputs_are_log_probs=True with labelled rows: the supervised gradient is -c_sup onehot(y), not c_sup (p - onehot)."""
    import torch
    for coeffs in ((1, 0, 0), oc.COEFFS[3]):
        _, parts, dz = _run(case, coeffs)
        assert int(parts["n_valid"]) == case.n_l - 1
        assert torch.count_nonzero(dz[:, 3]) == 0                                 # the ignore_index row
        assert int(torch.count_nonzero(dz[:, :case.n_l])) == case.S * (case.n_l - 1)   # one element per valid row and sample


@pytest.mark.parametrize("case", oc.SAMPLES, ids=oc.case_id)
def test_sample_counts_up_to_the_bound(case):
    _run(case)


def test_seventeen_samples_are_refused_by_the_wrapper():
    import torch
    from grand_plus_amd.objective import grand_plus_loss
    z = torch.zeros((oc.MAX_S + 1, 4, 3), device="cuda", requires_grad=True)
    with pytest.raises(ValueError, match="number of samples"):                    # the wrapper's own text: no native call was made
        grand_plus_loss(z, None, 0, 1.0)


@pytest.mark.parametrize("case", oc.CLASSES, ids=oc.case_id)
def test_class_counts_around_the_wave_width_and_at_the_bound(case):
    import torch
    loss, parts, dz = _run(case)
    if case.C == 1:                                                               # logp = 0, p = q = 1: nothing to learn
        assert float(parts["sup"]) == 0.0 and float(parts["con"]) == 0.0 and torch.count_nonzero(dz) == 0
    else:
        assert torch.count_nonzero(dz[:, :case.n_l]) > 0 and torch.count_nonzero(dz[:, case.n_l:]) > 0


def test_more_classes_than_the_bound_are_refused():
    import torch
    from grand_plus_amd.objective import grand_plus_loss
    z = torch.zeros((1, 2, oc.MAX_C + 1), device="cuda", requires_grad=True)
    with pytest.raises(ValueError, match="n_classes outside"):                    # GP_ERR_INVALID_ARG through raise_for_status
        grand_plus_loss(z, None, 0, 1.0)


@pytest.mark.parametrize("case", oc.ROWS, ids=oc.case_id)
def test_row_counts_below_one_workgroup_and_without_unlabelled_rows(case):
    loss, parts, dz = _run(case)
    if case.n_l == case.B:                                                        # no unlabelled row: L_con is a mean over nothing
        assert math.isnan(float(parts["con"])) and math.isnan(float(loss)) and int(parts["n_conf"]) == 0
        assert math.isfinite(float(parts["sup"]))
        assert oc.grad_error(dz, oc.reference(case, (0, 1, 0))["grad"])[1] <= 1.0  # the supervised gradient alone
    if case.n_l == 0:
        assert math.isnan(float(parts["sup"])) and math.isnan(float(loss))


def test_a_second_grid_stride_trip():
    """B = 65 535 * 4 + 37: the grid is capped, so the last 37 rows are the second trip of the loops over rows."""
    import torch
    case = oc.SECOND_TRIP
    _, _, dz = _run(case)
    gref = oc.reference(case)["grad"][:, -37:]
    assert torch.count_nonzero(gref) > 0 and torch.count_nonzero(dz[:, -37:]) > 0
    assert oc.grad_error(dz[:, -37:], gref)[1] <= 1.0


def test_no_rows_at_all():
    import torch
    from grand_plus_amd.objective import grand_plus_loss
    z = torch.zeros((2, 0, 7), device="cuda", requires_grad=True)
    loss, parts = grand_plus_loss(z, None, 0, 1.0)
    loss.backward()
    assert math.isnan(float(loss)) and math.isnan(float(parts["sup"])) and math.isnan(float(parts["con"]))
    assert [int(parts[k]) for k in ("n_conf", "n_valid", "n_correct", "n_bad_labels")] == [0, 0, 0, 0]
    assert z.grad is not None and tuple(z.grad.shape) == (2, 0, 7)


@pytest.mark.parametrize("case", oc.SHARPEN, ids=oc.case_id)
def test_sharpening_where_fp32_pow_underflows(case):
    """avg_p ** (1 / tem) ~ 2^-240 is 0 in fp32: the reference's own form gives 0 / 0 there, the kernels' log-domain form
    must not.  n_l = 0, so L_sup and the loss are NaN as always; L_con and dz are finite and match float64."""
    import torch
    z, _, _, conf = oc.build(case)
    lps = [torch.log_softmax(z[s], -1) for s in range(case.S)]
    assert math.isnan(float(consis_loss_ref(lps, case.tem, conf, case.kind)))     # why the case exists
    loss, parts, dz = _run(case)
    assert math.isfinite(float(parts["con"])) and bool(torch.isfinite(dz).all()) and float(dz.abs().max()) > 0
    assert int(parts["n_conf"]) == case.B


def test_argmax_ties_go_to_the_first_index():
    """Two or three columns share the last sample's row maximum: within a lane (c, c + 64), across adjacent lanes,
    lanes 0 and 63, the third stride against column 0.  n_correct follows torch.argmax: the first index."""
    import torch
    case = oc.TIES
    z, labels, n_l, _ = oc.build(case)
    _, parts, _ = _run(case)
    assert int(parts["n_correct"]) == int((torch.argmax(z[case.S - 1, :n_l], 1) == labels[:n_l]).sum()) == 3


def test_a_labelled_row_of_minus_infinity_logits_but_two():
    import torch
    _, parts, dz = _run(oc.NEGINF)
    assert bool(torch.isfinite(dz).all()) and int(torch.count_nonzero(dz[:, 2])) == 2 * oc.NEGINF.S
    assert math.isfinite(float(parts["sup"])) and math.isfinite(float(parts["con"]))


@pytest.mark.parametrize("layout", ["transposed", "padded"])
def test_strided_input_sends_the_gradient_to_its_base(layout):
    import torch
    from grand_plus_amd.objective import grand_plus_loss
    case = oc.STRIDED
    z, labels, n_l, conf = oc.build(case)
    ref = oc.reference(case)
    if layout == "transposed":
        base = z.transpose(0, 1).contiguous().cuda().requires_grad_(True)         # [B, S, C]
        zin = base.transpose(0, 1)
    else:
        pad = torch.randn((case.S, case.B, 3), generator=torch.Generator().manual_seed(1))
        base = torch.cat([z, pad], dim=-1).cuda().requires_grad_(True)            # [S, B, C + 3]
        zin = base[..., :case.C]
    assert not zin.is_contiguous()
    loss, parts = grand_plus_loss(zin, labels.cuda(), n_l, case.w, tem=case.tem, conf=conf, kind=case.kind)
    loss.backward()
    got = base.grad.transpose(0, 1) if layout == "transposed" else base.grad[..., :case.C]
    oc.assert_matches({"loss": loss, "sup": parts["sup"], "con": parts["con"]}, got, ref, f"strided, {layout}")
    if layout == "padded":
        assert torch.count_nonzero(base.grad[..., case.C:]) == 0


def test_two_runs_are_bitwise_equal():
    import torch
    from grand_plus_amd.objective import grand_plus_loss
    z, g = _logits(4, 3000, 100, seed=14)
    labels = torch.randint(0, 100, (500,), generator=g).cuda()
    res = []
    for _ in range(2):
        zc = z.cuda().requires_grad_(True)
        loss, parts = grand_plus_loss(zc, labels, 500, 0.8, tem=0.1, kind="kl")
        loss.backward()
        res.append((loss.detach().clone(), parts["sup"].detach().clone(), parts["con"].detach().clone(), zc.grad.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_step_does_not_synchronise_and_the_reference_does():
    import torch
    import torch.nn.functional as Fn
    from grand_plus_amd.objective import grand_plus_loss
    z, g = _logits(2, 250, 41, seed=15)
    labels = torch.randint(0, 41, (50,), generator=g).cuda()
    outs = [z[s].cuda().requires_grad_(True) for s in range(2)]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, parts = grand_plus_loss(outs, labels, 50, 1.0, tem=0.1, kind="kl")
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert all(o.grad is not None for o in outs)
    torch.cuda.set_sync_debug_mode("error")                                      # the reference's boolean-mask indexing does sync
    try:
        with pytest.raises(RuntimeError):
            lps = [torch.log_softmax(o.detach(), -1) for o in outs]
            consis_loss_ref([lp[50:] for lp in lps], 0.1, 2.0 / 41, "kl") + Fn.nll_loss(lps[0][:50], labels)
    finally:
        torch.cuda.set_sync_debug_mode(0)


def test_cora_shaped_training_step_end_to_end():
    """gfpush_device -> batch_positions -> random_prop_rows(samples=2) -> 2-layer MLP with BatchNorm per sample ->
    grand_plus_loss -> backward, against the float64 reference pipeline under the same masks."""
    import torch
    import torch.nn.functional as Fn
    from grand_plus_amd import Graph, synth
    from grand_plus_amd.augment import random_prop_rows
    from grand_plus_amd.objective import grand_plus_loss
    from grand_plus_amd.recipes import make_coef
    from grand_plus_amd.rows import RowMatrix
    from oracle.random_prop_ref import random_prop_ref
    indptr, indices = synth.shape_csr("tiny")
    n = len(indptr) - 1
    seeds = synth.seeds(n, 400)
    K, F, H, C, p_node, S = 32, 1433, 32, 7, 0.5, 2
    g = Graph(indptr, indices, 0)
    rm = RowMatrix.compute(g, seeds, make_coef("ppr", 6, 0.2), 1e-5, K)
    gen = torch.Generator().manual_seed(1)
    X = (torch.rand((n, F), generator=gen) < 0.02).float()                       # sparse binary bag-of-words, as Cora's
    batch_nodes = torch.from_numpy(np.asarray(seeds[:150], dtype=np.int64))      # 50 labelled + 100 unlabelled (run_cora.sh)
    n_l = 50
    labels = torch.randint(0, C, (n_l,), generator=gen)
    S_rows = len(seeds)
    keep = (torch.rand((S, S_rows * K), generator=gen) >= p_node).to(torch.uint8)
    lin1 = torch.nn.Linear(F, H); lin2 = torch.nn.Linear(H, C)
    for m in (lin1, lin2):
        m.weight.data = torch.randn(m.weight.shape, generator=gen) * 0.3
        m.bias.data = torch.randn(m.bias.shape, generator=gen) * 0.1
    bn_w = torch.rand((H,), generator=gen) + 0.5
    bn_b = torch.randn((H,), generator=gen) * 0.1
    w, tem = 0.8, 0.5

    def mlp(x, p):
        h = x @ p["w1"].t() + p["b1"]
        h = Fn.batch_norm(h, None, None, p["g"], p["beta"], training=True)
        return torch.relu(h) @ p["w2"].t() + p["b2"]

    init = {"w1": lin1.weight.data, "b1": lin1.bias.data, "g": bn_w, "beta": bn_b, "w2": lin2.weight.data, "b2": lin2.bias.data}
    # this project's path
    P = {k: v.cuda().clone().requires_grad_(True) for k, v in init.items()}
    rows = rm.batch_positions(batch_nodes.cuda(), check=False)
    aug = random_prop_rows(X.cuda(), rm.col, rm.val, rm.filled, K, batch_rows=rows, dropnode_rate=p_node, training=True,
                           keep=keep.cuda(), samples=S)
    logits = [mlp(aug[s], P) for s in range(S)]
    loss, parts = grand_plus_loss(logits, labels.cuda(), n_l, w, tem=tem, kind="l2")
    loss.backward()

    # float64 reference under the same masks: the flattened rows of the batch (model.py:310-316)
    idx, cols, scores, kp = rows_to_coo(rm.col.cpu(), rm.val.cpu(), rm.filled.cpu(), K, rows.cpu(), keep)
    R = {k: v.double().clone().requires_grad_(True) for k, v in init.items()}
    z_ref = torch.stack([mlp(random_prop_ref(X.double()[cols], scores.double(), idx, p_node, True, kp[s]), R) for s in range(S)])
    loss_r, _, _ = grand_loss_ref(z_ref, labels, n_l, w, tem, 2.0 / C, "l2")
    loss_r.backward()
    assert abs(float(loss) - float(loss_r)) <= 1e-5 * abs(float(loss_r)) + 1e-7
    top = max(float(R[k].grad.abs().max()) for k in init)
    for k in init:
        ref = R[k].grad
        scale = float(ref.abs().max())
        if k == "b1":                                                            # BatchNorm cancels the first bias: its
            assert scale <= 1e-12 * top                                          # gradient is 0 up to rounding on both sides
            assert float(P[k].grad.abs().max()) <= 1e-6 * top
            continue
        assert scale > 0, k
        torch.testing.assert_close(P[k].grad.double().cpu(), ref, rtol=1e-4, atol=1e-5 * scale)


def test_mag_shaped_training_step_with_two_samples():
    """test_gpu_embedding.py's MAG-shaped step with samples=2 and grand_plus_loss(kind="l2").  input_droprate = 0 (as
    run_mag.sh): the S-sample call shares one embedding output across the samples, where model_mag.py:355 recomputes it
    per sample -- with input dropout off those are the same computation."""
    import scipy.sparse as sp
    import torch
    import torch.nn.functional as Fn
    from grand_plus_amd import Graph, synth
    from grand_plus_amd.augment import random_prop
    from grand_plus_amd.embedding import embedding_bag_csr, flatten_rows
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
    gen = torch.Generator().manual_seed(0)
    W0 = torch.randn((V, H), generator=gen) * 0.1
    fw0 = torch.randn((C, H), generator=gen) * 0.2
    batch_rows = torch.arange(0, 40, dtype=torch.int32).cuda()                  # 20 labelled + 20 unlabelled (run_mag.sh)
    n_train = 20
    labels = torch.randint(0, C, (n_train,), generator=gen)
    nbr, scores, mat_idx = flatten_rows(col, val, filled, K, batch_rows)
    M = nbr.numel()
    keep = (torch.rand((S, M), generator=gen) >= p_node).to(torch.uint8)
    n_out = 40

    W = W0.cuda().requires_grad_(True)
    fw = fw0.cuda().requires_grad_(True); fb = torch.zeros(C, device="cuda", requires_grad=True)
    emb = embedding_bag_csr(W, ip, ix, dt, nodes=nbr, input_droprate=0.0, training=True)
    aug = random_prop(emb, scores, mat_idx, p_node, training=True, keep=keep.cuda(), samples=S, n_out=n_out)
    logits = [Fn.relu(aug[s]) @ fw.t() + fb for s in range(S)]
    loss, parts = grand_plus_loss(logits, labels.cuda(), n_train, 1.0, tem=0.5, conf=0.0, kind="l2")
    loss.backward()

    sub = A[nbr.cpu().numpy()]
    node_idx, attr_idx = sub.nonzero()
    node_idx, attr_idx = torch.from_numpy(node_idx.astype(np.int64)), torch.from_numpy(attr_idx.astype(np.int64))
    data = torch.from_numpy(sub.data).double()
    Wr = W0.double().requires_grad_(True)
    fwr = fw0.double().requires_grad_(True); fbr = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    num = torch.zeros((M, H), dtype=torch.float64).index_add_(0, node_idx, Wr[attr_idx] * data[:, None])
    den = torch.zeros((M, 1), dtype=torch.float64).index_add_(0, node_idx, data[:, None])
    emb_r = num / (den + 1e-10)                                                  # MLP.emb, model_mag.py:48-55 (no dropout)
    z_ref = torch.stack([Fn.relu(random_prop_ref(emb_r, scores.cpu().double(), mat_idx.cpu(), p_node, True, keep[s])) @ fwr.t() + fbr
                         for s in range(S)])
    loss_r, _, _ = grand_loss_ref(z_ref, labels, n_train, 1.0, 0.5, 0.0, "l2")
    loss_r.backward()
    assert abs(float(loss) - float(loss_r)) <= 1e-5 * abs(float(loss_r)) + 1e-7
    for got, ref in ((W.grad, Wr.grad), (fw.grad, fwr.grad), (fb.grad, fbr.grad)):
        scale = float(ref.abs().max())
        assert scale > 0
        torch.testing.assert_close(got.double().cpu(), ref, rtol=1e-4, atol=1e-5 * scale)
