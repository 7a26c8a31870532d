"""The device-resident step state and the captured training step on the GPU (cases in tests/step_cases.py).

The contract is bitwise: a replayed step equals the eager step of the same TrainStep body (`capture=False`), and the
masks written from the device seed equal the hash the existing kernels draw from `step_seed(base, t)`.  Only Adam's two
bias corrections may differ from the host-number step, by one float32 rounding (the device's double pow against the
host's); that comparison takes §7g's rule from tests/optim_cases.py."""
import copy
import math
import types

import numpy as np
import pytest
import torch

import optim_cases as oc
import step_cases as sc
from mag_cases import node_keep
from mlp_block_cases import hashed_keep

pytestmark = pytest.mark.gpu

TAIL = 4096


def _bits(a):
    a = a.detach().contiguous()
    return a.view(torch.int32) if a.dtype == torch.float32 else a


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _assert_twins(a, b, what):
    (ra, ma, oa), (rb, mb, ob) = a, b
    for name, x, y in zip(ra._fields, ra, rb):
        assert _same(x, y), f"{what}: {name} differs: {x.item()} vs {y.item()}"
    for i, (x, y) in enumerate(zip(sc.snapshot(ma, oa), sc.snapshot(mb, ob))):
        assert _same(x, y), f"{what}: tensor {i} of the snapshot differs"


def _ulps(a, b):
    return int(abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32))))


# ---- 1. the state
def test_advance_gives_tick_seed_weight_and_bias_corrections():
    """tick, seed and weight exactly; step_size and rsqrt_bc2 for t = 1 ... 300 within one float32 ulp of the host's
    lr / (1 - beta1**t) and 1 / sqrt(1 - beta2**t): both sides round a double that agrees to about 1e-13.
    Worst distance seen on the MI355X: see DESIGN §7m."""
    from grand_plus_amd import StepState
    from grand_plus_amd._common import step_seed
    from grand_plus_amd.step import step_weight
    betas = [(0.9, 0.999), (0.5, 0.9), (0.0, 0.999)]
    lrs = [1e-2, 1e-3, 0.05]
    opt = types.SimpleNamespace(param_groups=[{"lr": lr, "betas": b} for lr, b in zip(lrs, betas)])
    st = StepState("cuda", sc.BASE_SEED, sc.LAM, sc.WARMUP)
    assert st.read().tick == 0 and st.weight.dim() == 0 and st.weight.dtype == torch.float32
    worst = 0
    for t in range(1, 301):
        st.advance(opt)
        s = st.read()
        assert s.tick == t and s.seed == step_seed(sc.BASE_SEED, t)
        if t <= sc.WARMUP + 3:
            assert s.weight.view(np.int32) == step_weight(sc.LAM, sc.WARMUP, t).view(np.int32)
            assert float(st.weight) == float(s.weight)
        for g, (lr, (b1, b2)) in enumerate(zip(lrs, betas)):
            worst = max(worst, _ulps(s.step_size[g], lr / (1.0 - b1 ** t)), _ulps(s.rsqrt_bc2[g], 1.0 / math.sqrt(1.0 - b2 ** t)))
        assert not s.step_size[3:].any() and not s.rsqrt_bc2[3:].any()          # groups that do not exist stay untouched
    print(f"worst ulp distance of step_size / rsqrt_bc2 over t = 1..300: {worst}")
    assert worst <= 1
    assert s.weight == np.float32(sc.LAM)
    for lam, warmup in ((0.0, 5), (0.7, 1)):
        st = StepState("cuda", 3, lam, warmup)
        for t in range(1, warmup + 4):
            st.advance()
            s = st.read()
            assert s.tick == t and s.seed == step_seed(3, t)
            assert s.weight.view(np.int32) == step_weight(lam, warmup, t).view(np.int32)
            assert not s.step_size.any() and not s.rsqrt_bc2.any()
    st.set_tick(41)
    st.advance()
    assert st.read().tick == 42 and st.read().seed == step_seed(3, 42)


# ---- 2. the masks
def _guarded(n):
    return torch.full((n + TAIL,), 0xAA, dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("S", [1, 2, 16])
@pytest.mark.parametrize("B", [2, 37])
@pytest.mark.parametrize("p", [0.5, 1.0])
def test_masks_equal_the_host_hash_and_stay_in_their_slots(S, B, p):
    """One launch over a rows segment and four layer segments (F = 1, 33, 64, 65), at step t = 2, against the host mirrors
    of the hash under step_seed(base, 2); a p = 0 segment in the same call is left alone.  Every byte outside the batch's
    filled slots, and a 4 KiB tail behind every buffer, keeps its 0xAA."""
    from grand_plus_amd import StepState
    from grand_plus_amd._common import step_seed
    from grand_plus_amd.step import layer_segment, rows_segment, step_masks
    rm, _X, _y = sc.resident()
    filled = sc.problem()[3].numpy()
    empty, short, full = (int(np.flatnonzero(filled == f)[0]) for f in (0, 3, 8))
    rng = np.random.default_rng(B)
    rows = [short, empty] if B == 2 else [full, empty, short, full] + rng.choice(sc.S_ROWS, B - 4).tolist()   # `full` twice
    batch_rows = torch.tensor(rows, dtype=torch.int32, device="cuda")
    L = sc.S_ROWS * sc.K
    st = StepState("cuda", sc.BASE_SEED, sc.LAM, sc.WARMUP)
    st.advance()
    st.advance()
    seed = step_seed(sc.BASE_SEED, 2)
    widths = (1, 33, 64, 65)
    node = _guarded(S * L)
    layers = [_guarded(S * B * F) for F in widths]
    skipped = _guarded(S * B * 7)
    segs = [rows_segment(node[:S * L].view(S, L), batch_rows, rm.filled, sc.K, S, p)]
    segs += [layer_segment(buf[:S * B * F].view(S, B, F), l, p) for l, (buf, F) in enumerate(zip(layers, widths))]
    segs.insert(2, layer_segment(skipped[:S * B * 7].view(S, B, 7), 7, 0.0))
    step_masks(st, segs)
    torch.cuda.synchronize()

    want = torch.full((S, L), 0xAA, dtype=torch.uint8)
    ref = node_keep(seed, S, L, p)
    for r in set(rows):
        lo, hi = r * sc.K, r * sc.K + min(int(filled[r]), sc.K)
        want[:, lo:hi] = ref[:, lo:hi]
    got = node.cpu()
    assert torch.equal(got[:S * L].view(S, L), want)
    assert bool((got[S * L:] == 0xAA).all())
    if p == 1.0:
        assert not bool(want[want != 0xAA].any())                                # p = 1 writes zeros
    for l, (buf, F) in enumerate(zip(layers, widths)):
        got = buf.cpu()
        assert torch.equal(got[:S * B * F].view(S, B, F), hashed_keep(seed, l, S, B, F, p)), (l, F)
        assert bool((got[S * B * F:] == 0xAA).all())
    assert bool((skipped == 0xAA).all())                                         # p = 0 draws nothing
    assert st.read().tick == 2                                                   # the masks read the state, they do not move it


# ---- 3. forward equivalence
def test_masked_forward_equals_the_seeded_forward_bit_for_bit():
    from grand_plus_amd import StepState
    from grand_plus_amd._common import step_seed
    from grand_plus_amd.augment import random_prop_rows
    from grand_plus_amd.step import layer_segment, rows_segment, step_masks
    rm, X, _y = sc.resident()
    S, B = 2, 32
    st = StepState("cuda", sc.BASE_SEED, sc.LAM, sc.WARMUP)
    rows = torch.from_numpy(np.random.default_rng(0).choice(sc.S_ROWS, B).astype(np.int32)).cuda()
    models = {name: sc.model(name) for name in sc.LAYOUTS}
    for t in (1, 2):
        st.advance()
        seed = step_seed(sc.BASE_SEED, t)
        node = torch.zeros((S, sc.S_ROWS * sc.K), dtype=torch.uint8, device="cuda")
        step_masks(st, [rows_segment(node, rows, rm.filled, sc.K, S, sc.P_NODE)])
        args = (X, rm.col, rm.val, rm.filled, sc.K)
        kw = dict(batch_rows=rows, dropnode_rate=sc.P_NODE, training=True, samples=S)
        a = random_prop_rows(*args, keep=node, seed=0, **kw)
        b = random_prop_rows(*args, seed=seed, **kw)
        assert _same(a, b), t
        for name, m in models.items():
            ref = copy.deepcopy(m)
            keeps = [torch.zeros((S, B, fc.weight.shape[1]), dtype=torch.uint8, device="cuda") if p > 0 else None
                     for fc, _bn, _r, _n, _d, p in m._layers()]
            step_masks(st, [layer_segment(k, l, m._layers()[l][5]) for l, k in enumerate(keeps) if k is not None])
            with torch.no_grad():
                assert _same(m(a, seed=0, keep=keeps), ref(b, seed=seed)), (name, t)


# ---- 4. the capturable optimiser
def _state_of(opt, params):
    return {"param": [p.detach() for p in params], "exp_avg": [opt.state[p]["exp_avg"] for p in params],
            "exp_avg_sq": [opt.state[p]["exp_avg_sq"] for p in params]}


def test_capturable_clipadam_follows_the_reference_and_checkpoints_both_ways():
    """5 eager steps on the cora set of optim_cases under the sync debug mode, held to §7g's rule; then the checkpoint
    goes into a host-number ClipAdam, into torch.optim.Adam and back into a capturable one: step == 5 everywhere."""
    from grand_plus_amd import ClipAdam, StepState
    hi = 0
    h = oc.HYPERS[hi]
    init, seq = oc.inputs("cora", hi)
    r64, t32 = oc.reference("cora", hi)
    params = oc.device_params("cora", init)
    dev_seq = [[g.cuda() for g in grads] for grads in seq]
    kw = dict(lr=h["lr"], betas=oc.BETAS, eps=oc.EPS, weight_decay=h["weight_decay"], clip_norm=h["clip"])
    st = StepState("cuda", 1, 1.0, 10)
    opt = ClipAdam(params, capturable=True, state=st, **kw)
    norms = []
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for grads in dev_seq:
            st.advance(opt)
            for p, g in zip(params, grads):
                p.grad = g
            norms.append(opt.step())
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    oc.error_ratios(_state_of(opt, params), t32, r64, "capturable cora-h0")
    host_params = oc.device_params("cora", init)                                 # the host-number ClipAdam, same gradients
    host_opt = ClipAdam(host_params, **kw)
    for grads in dev_seq:
        for p, g in zip(host_params, grads):
            p.grad = g
        host_opt.step()
    oc.error_ratios(_state_of(host_opt, host_params), t32, r64, "host-number cora-h0")
    print("capturable == host-number, bit for bit:", all(_same(p, q) for p, q in zip(params, host_params)))
    for got, ref in zip(norms, r64["norm"]):
        assert abs(float(got) - float(ref)) <= 2.0 ** -23 * float(ref)
    assert all(not isinstance(opt.state[p]["step"], torch.Tensor) for p in params)
    sd = opt.state_dict()
    assert [s["step"] for s in sd["state"].values()] == [5] * len(params) and st.read().tick == 5

    plain = ClipAdam(params, **kw)                                               # capturable -> host-number ClipAdam
    plain.load_state_dict(copy.deepcopy(sd))
    assert all(plain.state[p]["step"] == 5 for p in params)
    adam = torch.optim.Adam(params, lr=h["lr"], betas=oc.BETAS, eps=oc.EPS, weight_decay=h["weight_decay"], foreach=False)
    adam.load_state_dict(copy.deepcopy(sd))                                      # capturable -> torch.optim.Adam
    assert all(float(adam.state[p]["step"]) == 5 for p in params)
    for source in (plain, adam):                                                 # ... and back
        st2 = StepState("cuda", 1, 1.0, 10)
        back = ClipAdam(params, capturable=True, state=st2, **kw)
        back.load_state_dict(copy.deepcopy(source.state_dict()))
        assert st2.read().tick == 5
        assert [s["step"] for s in back.state_dict()["state"].values()] == [5] * len(params)
    # a sixth step of the reloaded optimiser is step 6 of Adam: the host-number twin takes the same step
    twin = [torch.nn.Parameter(p.detach().clone()) for p in params]
    plain2 = ClipAdam(twin, **kw)
    sd_twin = copy.deepcopy(sd)
    plain2.load_state_dict(sd_twin)
    for p, q, g in zip(params, twin, dev_seq[0]):
        p.grad, q.grad = g, g.clone()
    st2.advance(back)
    back.step()
    plain2.step()
    assert st2.read().tick == 6 and all(plain2.state[q]["step"] == 6 for q in twin)
    # one ulp of each bias correction on an update of at most a few lr, then one rounding of the parameter itself
    top = max(float(p.detach().abs().max()) for p in params)
    for p, q in zip(params, twin):
        torch.testing.assert_close(p, q, rtol=0, atol=2.0 ** -23 * (8 * h["lr"] + top))


# ---- 5. the eager twin against the host-number step
def test_eager_twin_equals_the_host_number_step():
    """Logits and dz bit for bit at step 1; parameters and Adam's moments after 6 steps inside §7g's rule against the
    float64 reference fed the host-number run's gradients (one ulp of bias correction is all that may differ)."""
    from grand_plus_amd.step import trained_parameters
    name = "cora"
    res = sc.resident()
    rm, X, labels = res
    ts, m, opt = sc.train_step(name, capture=False, resident_=res)
    hm = sc.model(name)
    hps = trained_parameters(hm)
    hopt = sc.optimizer(hps, False)
    init = [p.detach().cpu().clone() for p in hps]
    seen = {}

    def grab(tag):
        def hook(_mod, _inp, out):
            seen.setdefault(tag, []).append(out.detach().clone())
            out.register_hook(lambda g: seen.setdefault(tag + "_dz", []).append(g.detach().clone()))
        return hook

    m.register_forward_hook(grab("twin"))
    hm.register_forward_hook(grab("host"))
    seq = []
    for t in range(1, 7):
        sel = sc.selection(t)
        ts.step(*sel)
        seq.append(sc.host_step(hm, hopt, rm, X, labels, ts._pos, t, sel, name))
        if t == 1:
            assert _same(seen["twin"][0], seen["host"][0]) and _same(seen["twin_dz"][0], seen["host_dz"][0])
    assert ts.state.read().tick == 6 and all(hopt.state[p]["step"] == 6 for p in hps)
    r64 = oc.torch_run(init, seq, sc.HYPER, torch.float64)
    t32 = oc.torch_run(init, seq, sc.HYPER, torch.float32)
    oc.error_ratios(_state_of(opt, trained_parameters(m)), t32, r64, "eager twin")
    oc.error_ratios(_state_of(hopt, hps), t32, r64, "host-number step")


# ---- 6. replay against the eager twin: the contract
def _twins(name, S=2):
    res = sc.resident()
    return sc.train_step(name, capture=True, S=S, resident_=res), sc.train_step(name, capture=False, S=S, resident_=res)


@pytest.mark.parametrize("name,S", [("cora", 2), ("reddit", 2), ("pubmed", 2), ("cora", 16)])
def test_replay_equals_the_eager_twin_bit_for_bit(name, S):
    (cap, cm, co), (eag, em, eo) = _twins(name, S)
    losses = []
    for t in range(1, 9):
        sel = sc.selection(3 if t == 4 else t)                                   # steps 3 and 4 get the same selection
        rc, re = cap.step(*sel), eag.step(*sel)
        _assert_twins((rc, cm, co), (re, em, eo), f"{name} S={S} step {t}")
        losses.append(float(rc.loss))
    assert cap.state.read().tick == eag.state.read().tick == 8
    assert len(cap._shapes) == 1 and cap._shapes[(32, 8)] is not None and not eag._shapes
    assert all(math.isfinite(x) for x in losses)
    assert losses[2] != losses[3], "the same selection gave the same loss: the masks did not advance inside the replay"


# ---- 7. shapes
def test_a_ragged_batch_gets_its_own_graph_and_a_fifth_shape_runs_eagerly():
    (cap, cm, co), (eag, em, eo) = _twins("reddit")
    shapes = [(8, 24), (8, 24), (8, 24), (5, 11), (5, 11), (8, 24), (5, 11), (8, 20), (8, 20), (3, 24), (3, 24),
              (6, 6), (6, 6), (6, 6), (8, 24)]
    for t, (n_l, n_u) in enumerate(shapes, start=1):
        sel = sc.selection(t, n_l, n_u)
        _assert_twins((cap.step(*sel), cm, co), (eag.step(*sel), em, eo), f"step {t} shape {(n_l, n_u)}")
        if t == 3:
            first = cap._shapes[(32, 8)]
        if t == 5:
            assert len(cap._shapes) == 2 and cap._shapes[(16, 5)] is not None     # the ragged batch: a second graph
        if t == 6:
            assert cap._shapes[(32, 8)] is first                                  # back to the first shape: its graph replays
    assert sorted(cap._shapes) == [(16, 5), (27, 3), (28, 8), (32, 8)] and all(v is not None for v in cap._shapes.values())
    assert (12, 6) not in cap._shapes                                             # the fifth shape ran eagerly, three times
    tick = cap.state.read().tick
    assert tick == len(shapes)
    before = sc.snapshot(cm, co)
    for bad in ((np.array([0, sc.N_TRAIN]), np.array([1])), (np.array([-1]), np.array([1])),
                (np.array([0]), np.array([sc.S_ROWS - sc.N_TRAIN]))):
        for ts in (cap, eag):
            with pytest.raises(IndexError):
                ts.step(*bad)
    assert cap.state.read().tick == tick == eag.state.read().tick
    assert all(_same(a, b) for a, b in zip(before, sc.snapshot(cm, co)))


# ---- 8. no synchronisation, no disturbance
def test_a_replayed_step_does_not_synchronise_and_valid_between_steps_changes_nothing():
    from grand_plus_amd import valid
    (cap, cm, co), (eag, em, eo) = _twins("reddit")
    rm, X, labels = sc.resident()
    idx_val = sc.pools()[1][:30]
    for t in range(1, 4):
        sel = sc.selection(t)
        _assert_twins((cap.step(*sel), cm, co), (eag.step(*sel), em, eo), f"step {t}")
    outs = []
    for ts, m in ((cap, cm), (eag, em)):
        before = ts.state.read()
        outs.append(valid(m, ts.rows, ts.features, idx_val, labels))
        assert m.training and ts.state.read().tick == before.tick == 3
    assert _same(outs[0][0], outs[1][0]) and _same(outs[0][1], outs[1][1])
    sels = [sc.selection(t) for t in range(4, 7)]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = [tuple(x.clone() for x in cap.step(*sel)) for sel in sels]          # replays: nothing may wait for the GPU
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    for sel, rc in zip(sels, got):
        re = eag.step(*sel)
        for name, x, y in zip(re._fields, rc, re):
            assert _same(x, y), name
    _assert_twins((cap.step(*sc.selection(7)), cm, co), (eag.step(*sc.selection(7)), em, eo), "step 7")
