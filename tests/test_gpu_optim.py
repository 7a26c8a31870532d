"""ClipAdam and clip_grad_norm against torch's own clip_grad_norm_ + Adam(foreach=False) on the CPU in float64
(tests/optim_cases.py).  The error bound is not a fixed number: ours may be off the float64 run by at most 4 times what
torch's float32 CPU run is off on the same inputs, plus one ulp of the largest value.  The norm is held to one float32
rounding of the float64 norm: the squares are exact in float64, the float64 sum's error is negligible at these sizes,
then one sqrt and one rounding."""
import copy
import re

import pytest
import torch

import optim_cases as oc

pytestmark = pytest.mark.gpu

CASES = oc.GRID
IDS = [f"{name}-h{hi}" for name, hi in CASES]


def _optimizer(params, hi, **kw):
    from grand_plus_amd import ClipAdam
    h = oc.HYPERS[hi]
    return ClipAdam(params, lr=h["lr"], betas=oc.BETAS, eps=oc.EPS, weight_decay=h["weight_decay"], clip_norm=h["clip"], **kw)


def _state_of(opt, params):
    state = [opt.state.get(p, {}) for p in params]
    return {"param": [p.detach() for p in params], "exp_avg": [s.get("exp_avg") for s in state],
            "exp_avg_sq": [s.get("exp_avg_sq") for s in state]}


def _run(name, hi, steps=oc.STEPS):
    """`steps` steps of ClipAdam over the case's gradient sequence: (params, optimizer, norms)."""
    init, seq = oc.inputs(name, hi)
    params = oc.device_params(name, init)
    opt = _optimizer(params, hi)
    norms = []
    for grads in seq[:steps]:
        oc.set_grads(params, grads)
        norms.append(opt.step())
    return params, opt, norms


def _assert_norm(norm, ref64):
    ref = float(ref64)
    assert norm.dtype == torch.float32 and norm.dim() == 0 and norm.is_cuda
    assert abs(float(norm) - ref) <= 2.0 ** -23 * ref, (float(norm), ref)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.detach().contiguous().view(torch.int32), b.detach().contiguous().view(torch.int32))


@pytest.mark.parametrize("name,hi", CASES, ids=IDS)
def test_five_steps_match_the_float64_reference_within_torchs_own_float32_error(name, hi):
    """Parameters, exp_avg and exp_avg_sq after 5 steps, and the norm of every step.  Ratios ours / torch32 seen on the
    MI355X are listed in DESIGN §7g."""
    r64, t32 = oc.reference(name, hi)
    params, opt, norms = _run(name, hi)
    oc.error_ratios(_state_of(opt, params), t32, r64, f"{name}-h{hi}")
    for got, ref in zip(norms, r64["norm"]):
        _assert_norm(got, ref)
    for p in params:
        if p in opt.state:
            assert opt.state[p]["step"] == oc.STEPS and not isinstance(opt.state[p]["step"], torch.Tensor)


@pytest.mark.parametrize("name", ["cora", "odd", "views", "many"])
def test_two_runs_from_equal_state_give_equal_bits(name):
    a_params, a_opt, a_norms = _run(name, 0, steps=3)
    b_params, b_opt, b_norms = _run(name, 0, steps=3)
    a, b = _state_of(a_opt, a_params), _state_of(b_opt, b_params)
    for key in a:
        for x, y in zip(a[key], b[key]):
            assert _bits_equal(x, y), key
    for x, y in zip(a_norms, b_norms):
        assert _bits_equal(x, y)


@pytest.mark.parametrize("name", ["many", "views"])
def test_a_tensor_stepped_alone_equals_the_same_tensor_inside_a_set(name):
    """Element independence, clipping off: the update of a tensor does not depend on its neighbours in the call, on the
    group of the table it lands in or on its alignment (alone it is a fresh, aligned allocation)."""
    hi = 1
    init, seq = oc.inputs(name, hi)
    params, opt, _ = _run(name, hi, steps=3)
    for i in ((0, 16, 31, 32, 39) if name == "many" else range(len(init))):
        solo = torch.nn.Parameter(init[i].cuda())
        assert solo.data_ptr() % 16 == 0
        solo_opt = _optimizer([solo], hi)
        for grads in seq[:3]:
            solo.grad = grads[i].cuda()
            solo_opt.step()
        assert _bits_equal(solo, params[i]), i
        assert _bits_equal(solo_opt.state[solo]["exp_avg"], opt.state[params[i]]["exp_avg"]), i
        assert _bits_equal(solo_opt.state[solo]["exp_avg_sq"], opt.state[params[i]]["exp_avg_sq"]), i


def test_step_leaves_the_gradients_unchanged_bit_for_bit():
    init, seq = oc.inputs("cora", 0)
    params = oc.device_params("cora", init)
    opt = _optimizer(params, 0)                                   # clipping active
    oc.set_grads(params, seq[0])
    before = [p.grad.clone() for p in params]
    opt.step()
    for p, g in zip(params, before):
        assert _bits_equal(p.grad, g)


def test_parameters_without_a_gradient_and_their_missing_state_are_untouched():
    init, seq = oc.inputs("holes", 0)
    params, opt, _ = _run("holes", 0, steps=2)
    for i, p in enumerate(params):
        if i in oc.HOLES:
            assert _bits_equal(p, init[i].cuda()) and p not in opt.state and p.grad is None
        else:
            assert set(opt.state[p]) == {"step", "exp_avg", "exp_avg_sq"} and not _bits_equal(p, init[i].cuda())


@pytest.mark.parametrize("name", ["cora", "odd", "views", "many"])
def test_clip_grad_norm_scales_by_the_fp32_coefficient_of_the_returned_norm(name):
    from grand_plus_amd import clip_grad_norm
    init, seq = oc.inputs(name, 0)
    params = oc.device_params(name, init)
    oc.set_grads(params, seq[0])
    before = [p.grad.clone() for p in params]
    max_norm = 0.1
    norm = clip_grad_norm(params, max_norm)
    _assert_norm(norm, oc.reference(name, 0)[0]["norm"][0])
    coef = torch.tensor(max_norm, dtype=torch.float32) / (norm.cpu() + torch.tensor(1e-6, dtype=torch.float32))
    assert coef.dtype == torch.float32 and float(coef) < 1.0
    for p, g in zip(params, before):
        assert _bits_equal(p.grad, g * coef.cuda())
    # large max_norm: the coefficient clamps to 1
    scaled = [p.grad.clone() for p in params]
    clip_grad_norm(params, 1e6)
    for p, g in zip(params, scaled):
        assert _bits_equal(p.grad, g)


def test_clip_grad_norm_where_the_1e6_of_the_coefficient_decides():
    """Gradients of total norm 1.1e-6 (the "odd" set at 1e-8) and max_norm = 2e-6: max_norm / (norm + 1e-6) is about 0.95,
    max_norm / norm about 1.8 and clamps to 1.  Bitwise against g * coef, after showing that the two coefficients differ."""
    from grand_plus_amd import clip_grad_norm
    hi = oc.TINY
    max_norm = oc.HYPERS[hi]["clip"]
    init, seq = oc.inputs("odd", hi)
    params = oc.device_params("odd", init)
    oc.set_grads(params, seq[0])
    before = [p.grad.clone() for p in params]
    norm = clip_grad_norm(params, max_norm)
    _assert_norm(norm, oc.reference("odd", hi)[0]["norm"][0])
    one, m = torch.tensor(1.0, dtype=torch.float32), torch.tensor(max_norm, dtype=torch.float32)
    coef = torch.minimum(m / (norm.cpu() + torch.tensor(1e-6, dtype=torch.float32)), one)
    without = torch.minimum(m / norm.cpu(), one)
    assert coef.dtype == torch.float32 and 0.5 < float(coef) < 1.0 and float(without) != float(coef)
    for p, g in zip(params, before):
        assert _bits_equal(p.grad, g * coef.cuda())
        assert g.numel() == 0 or not _bits_equal(p.grad, g * without.cuda())


def _off_default_ids():
    return [f"{name}-h{hi}" for name, hi, _, _ in oc.OFF_DEFAULT]


@pytest.mark.parametrize("capturable", [False, True], ids=["host_number", "capturable"])
@pytest.mark.parametrize("name,hi,betas,eps", oc.OFF_DEFAULT, ids=_off_default_ids())
def test_betas_and_eps_away_from_the_defaults(name, hi, betas, eps, capturable):
    """betas = (0.8, 0.99) and eps = 1e-6, five steps: through the host-number ClipAdam, whose step numbers the host forms,
    and through the capturable one, where step_state.hip forms the bias corrections from the device's tick."""
    from grand_plus_amd import ClipAdam, StepState
    h = oc.HYPERS[hi]
    init, seq = oc.inputs(name, hi)
    r64, t32 = oc.reference(name, hi, oc.STEPS, betas, eps)
    params = oc.device_params(name, init)
    kw = dict(lr=h["lr"], betas=betas, eps=eps, weight_decay=h["weight_decay"], clip_norm=h["clip"])
    st = StepState("cuda", 1, 1.0, 10) if capturable else None
    opt = ClipAdam(params, capturable=True, state=st, **kw) if capturable else ClipAdam(params, **kw)
    norms = []
    for grads in seq:
        if capturable:
            st.advance(opt)
        oc.set_grads(params, grads)
        norms.append(opt.step())
    oc.error_ratios(_state_of(opt, params), t32, r64, f"{name}-h{hi} betas {betas} eps {eps} capturable {capturable}")
    for got, ref in zip(norms, r64["norm"]):
        _assert_norm(got, ref)


def test_clip_grad_norm_with_max_norm_0_returns_the_norm_and_touches_nothing():
    from grand_plus_amd import clip_grad_norm
    init, seq = oc.inputs("odd", 0)
    params = oc.device_params("odd", init)
    oc.set_grads(params, seq[0])
    before = [p.grad.clone() for p in params]
    norm = clip_grad_norm(params, 0.0)
    _assert_norm(norm, oc.reference("odd", 0)[0]["norm"][0])
    for p, g, p0 in zip(params, before, init):
        assert _bits_equal(p.grad, g) and _bits_equal(p, p0.cuda())


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_gradients_spread_as_in_torchs_float32_path(bad):
    """One inf (the norm is inf, the coefficient 0, inf * 0 = NaN in that element alone) and one NaN (the norm and with it
    every element is NaN): the same pattern of non-finite entries as torch on the same inputs."""
    hi = 0
    init, seq = oc.inputs("odd", hi)
    grads = [g.clone() for g in seq[0]]
    grads[3][17] = bad
    t32 = oc.torch_run(init, [grads], oc.HYPERS[hi], torch.float32)
    params = oc.device_params("odd", init)
    opt = _optimizer(params, hi)
    oc.set_grads(params, grads)
    norm = opt.step().cpu()
    ref_norm = t32["norm"][0]
    assert bool(torch.isnan(norm)) == bool(torch.isnan(ref_norm)) and bool(torch.isinf(norm)) == bool(torch.isinf(ref_norm))
    n_bad = 0
    for p, q in zip(params, t32["param"]):
        assert torch.equal(torch.isnan(p).cpu(), torch.isnan(q)) and torch.equal(torch.isinf(p).cpu(), torch.isinf(q))
        n_bad += int((~torch.isfinite(q)).sum())
    assert n_bad == (1 if bad == float("inf") else sum(oc.numel(s) for s in oc.SETS["odd"]))


def _torch_adam(params, hi, lr=None):
    h = oc.HYPERS[hi]
    return torch.optim.Adam(params, lr=h["lr"] if lr is None else lr, betas=oc.BETAS, eps=oc.EPS, weight_decay=h["weight_decay"],
                            foreach=False)


def _torch_step(opt, params, hi):
    if oc.HYPERS[hi]["clip"] > 0:
        torch.nn.utils.clip_grad_norm_([p for p in params if p.grad is not None], oc.HYPERS[hi]["clip"], foreach=False)
    opt.step()


@pytest.mark.parametrize("name,hi", [("cora", 0), ("odd", 1)])
def test_a_torch_adam_checkpoint_continues_in_clipadam(name, hi):
    """3 steps of torch.optim.Adam on the GPU, its state_dict loaded into ClipAdam, 2 more steps: the 5-step reference."""
    init, seq = oc.inputs(name, hi)
    r64, t32 = oc.reference(name, hi)
    params = oc.device_params(name, init)
    adam = _torch_adam(params, hi)
    for grads in seq[:3]:
        oc.set_grads(params, grads)
        _torch_step(adam, params, hi)
    opt = _optimizer(params, hi)
    opt.load_state_dict(copy.deepcopy(adam.state_dict()))
    assert all(s["step"] == 3 and not isinstance(s["step"], torch.Tensor) for s in opt.state.values())
    for grads in seq[3:]:
        oc.set_grads(params, grads)
        opt.step()
    oc.error_ratios(_state_of(opt, params), t32, r64, f"adam->clipadam {name}-h{hi}")


@pytest.mark.parametrize("name,hi", [("cora", 0), ("odd", 1)])
def test_a_clipadam_checkpoint_continues_in_torch_adam(name, hi):
    init, seq = oc.inputs(name, hi)
    r64, t32 = oc.reference(name, hi)
    params, opt, _ = _run(name, hi, steps=3)
    adam = _torch_adam(params, hi)
    adam.load_state_dict(copy.deepcopy(opt.state_dict()))
    for group in adam.param_groups:
        group["foreach"] = False                                  # the loaded groups carry ClipAdam's foreach=None
    for grads in seq[3:]:
        oc.set_grads(params, grads)
        _torch_step(adam, params, hi)
    assert all(float(s["step"]) == 5 for s in adam.state.values())
    oc.error_ratios(_state_of(adam, params), t32, r64, f"clipadam->adam {name}-h{hi}")


def test_two_parameter_groups_with_different_lr_share_one_norm():
    """Groups {0, 1} at lr and {2, 3} at lr / 10 of cora, clipping active: one norm over all four, the update per group."""
    from grand_plus_amd import ClipAdam
    hi = 0
    h = oc.HYPERS[hi]
    init, seq = oc.inputs("cora", hi)

    def ref(dtype):
        ps = [torch.nn.Parameter(p.to(dtype).clone()) for p in init]
        opt = torch.optim.Adam([{"params": ps[:2]}, {"params": ps[2:], "lr": h["lr"] / 10}], lr=h["lr"], betas=oc.BETAS,
                               eps=oc.EPS, weight_decay=h["weight_decay"], foreach=False)
        norms = []
        for grads in seq:
            oc.set_grads(ps, [g.to(dtype) for g in grads])
            norms.append(torch.nn.utils.clip_grad_norm_(ps, h["clip"], foreach=False).clone())
            opt.step()
        out = _state_of(opt, ps)
        out["norm"] = norms
        return out

    r64, t32 = ref(torch.float64), ref(torch.float32)
    params = oc.device_params("cora", init)
    opt = ClipAdam([{"params": params[:2]}, {"params": params[2:], "lr": h["lr"] / 10}], lr=h["lr"], betas=oc.BETAS, eps=oc.EPS,
                   weight_decay=h["weight_decay"], clip_norm=h["clip"])
    for grads, ref_norm in zip(seq, r64["norm"]):
        oc.set_grads(params, grads)
        _assert_norm(opt.step(), ref_norm)
    oc.error_ratios(_state_of(opt, params), t32, r64, "two groups")


@pytest.mark.parametrize("make,msg", [
    (lambda: torch.full((6, 4), 0.5, dtype=torch.float64, device="cuda"), "must be float32, got torch.float64"),
    (lambda: torch.full((6, 4), 0.5, dtype=torch.float16, device="cuda"), "must be float32, got torch.float16"),
    (lambda: torch.full((4, 6), 0.5, device="cuda").t(), "must be contiguous, got strides (1, 6)"),
], ids=["float64", "half", "transposed"])
def test_cuda_parameters_the_kernels_cannot_read_are_refused_and_untouched(make, msg):
    """A half parameter read as float* would be read past its end: the refusal comes before any launch."""
    from grand_plus_amd import ClipAdam, clip_grad_norm
    good = torch.nn.Parameter(torch.full((5,), 0.5, device="cuda"))
    good.grad = torch.ones_like(good)
    bad = torch.nn.Parameter(make())
    bad.grad = torch.ones_like(bad)
    before = [good.detach().clone(), bad.detach().clone(), good.grad.clone(), bad.grad.clone()]
    opt = ClipAdam([good, bad], lr=1e-2, clip_norm=0.1)
    for run in (opt.step, lambda: clip_grad_norm([good, bad], 0.1)):
        with pytest.raises(TypeError, match=re.escape(msg)):
            run()
    assert len(opt.state) == 0
    for now, was in zip([good, bad, good.grad, bad.grad], before):
        assert torch.equal(now.detach(), was)


@pytest.mark.parametrize("bad,msg", [
    (lambda p: torch.zeros_like(p, dtype=torch.float16), "exp_avg_sq must be float32, got torch.float16"),
    (lambda p: torch.zeros(4, 6, device="cuda").t(), "exp_avg_sq must be contiguous"),
], ids=["half", "non-contiguous"])
def test_bad_loaded_state_is_refused_before_any_step_count_moves(bad, msg):
    """The second parameter's exp_avg_sq is wrong: the refusal leaves the first parameter's step count where it was."""
    from grand_plus_amd import ClipAdam
    ps = [torch.nn.Parameter(torch.zeros(3, device="cuda")), torch.nn.Parameter(torch.zeros(6, 4, device="cuda"))]
    for p in ps:
        p.grad = torch.ones_like(p)
    opt = ClipAdam(ps)
    for p in ps:
        opt.state[p] = {"step": 3, "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
    opt.state[ps[1]]["exp_avg_sq"] = bad(ps[1])
    with pytest.raises(TypeError, match=re.escape(msg)):
        opt.step()
    assert [opt.state[p]["step"] for p in ps] == [3, 3]
    assert all(float(p.abs().max()) == 0.0 for p in ps)


def test_no_gradients_give_a_zero_norm_on_the_parameters_device():
    from grand_plus_amd import ClipAdam, clip_grad_norm
    p = torch.nn.Parameter(torch.zeros(5, device="cuda"))
    opt = ClipAdam([p])
    for norm in (opt.step(), clip_grad_norm([p], 1.0)):
        assert norm.is_cuda and norm.dtype == torch.float32 and norm.dim() == 0 and float(norm) == 0.0
    assert len(opt.state) == 0


def test_views_have_unaligned_gradients_too():
    """The scalar branches of the norm kernel and of the clip-only path are taken on the gradient pointer alone."""
    init, seq = oc.inputs("views", 0)
    params = oc.device_params("views", init)
    oc.set_grads(params, seq[0])
    assert all(p.data_ptr() % 16 != 0 and p.grad.data_ptr() % 16 != 0 for p in params)
    assert all(_bits_equal(p.grad, g.cuda()) for p, g in zip(params, seq[0]))


def test_step_and_clip_grad_norm_do_not_synchronise_with_the_host():
    from grand_plus_amd import clip_grad_norm
    init, seq = oc.inputs("many", 0)
    params = oc.device_params("many", init)
    opt = _optimizer(params, 0)
    oc.set_grads(params, seq[0])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step()                                                # the step that creates the state
        opt.step()
        clip_grad_norm(params, 0.1)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()


def test_cora_shaped_training_step_end_to_end():
    """random_prop_rows(samples=2) -> GrandPlusMLP -> grand_plus_loss -> backward -> ClipAdam, beside the same model and
    seeds stepped by torch's clip_grad_norm_ + Adam.  The kernels are deterministic, so both see the same gradients bit
    for bit; one optimiser step is then held to the bound, the float64 reference fed those gradients."""
    import numpy as np
    from grand_plus_amd.augment import random_prop_rows
    from grand_plus_amd.mlp import GrandPlusMLP
    from grand_plus_amd.objective import grand_plus_loss
    hi = 0
    F, H, C, n_l, n_u, K, N, S_rows = 1433, 64, 7, 50, 100, 32, 2708, 400
    B = n_l + n_u
    rng = np.random.default_rng(3)
    col = torch.from_numpy(rng.integers(0, N, S_rows * K).astype(np.int32)).cuda()
    val = torch.from_numpy(np.sort(rng.random((S_rows, K)) ** 4, axis=1)[:, ::-1].copy().reshape(-1)).cuda()
    filled = torch.full((S_rows,), K, dtype=torch.int32, device="cuda")
    rows = torch.from_numpy(rng.choice(S_rows, B, replace=False).astype(np.int32)).cuda()
    gen = torch.Generator().manual_seed(4)
    X = (torch.rand((N, F), generator=gen) < 0.05).float().cuda()
    labels = torch.randint(0, C, (n_l,), generator=gen).cuda()
    torch.manual_seed(5)
    ours = GrandPlusMLP(F, C, H, 2, False, 0.5, 0.7, False).cuda().train()
    twin = copy.deepcopy(ours)

    def backward(model):
        aug = random_prop_rows(X, col, val, filled, K, batch_rows=rows, dropnode_rate=0.5, training=True, seed=77, samples=2)
        loss, _ = grand_plus_loss(model(aug, seed=78), labels, n_l, 1.0, tem=0.5, conf=0.0, kind="l2")
        loss.backward()

    backward(ours)
    backward(twin)
    ps = [p for p in ours.parameters() if p.grad is not None]
    qs = [q for q in twin.parameters() if q.grad is not None]
    assert len(ps) == len(qs) > 0
    for p, q in zip(ps, qs):
        assert _bits_equal(p.grad, q.grad)
    init = [p.detach().cpu().clone() for p in ps]
    grads = [p.grad.cpu().clone() for p in ps]
    r64 = oc.torch_run(init, [grads], oc.HYPERS[hi], torch.float64)
    t32 = oc.torch_run(init, [grads], oc.HYPERS[hi], torch.float32)

    opt = _optimizer(ours.parameters(), hi)
    norm = opt.step()
    _assert_norm(norm, r64["norm"][0])
    oc.error_ratios(_state_of(opt, ps), t32, r64, "end to end")
    adam = _torch_adam(qs, hi)
    _torch_step(adam, qs, hi)
    for p, q in zip(ps, qs):                                      # torch's own GPU step of the twin: fp32 neighbours
        torch.testing.assert_close(p, q, rtol=1.3e-6, atol=1e-5)
