"""MAG's captured training step with the table stepped from the backward's row list (DESIGN §7t,
`MagTrainStep(table_step=...)`), at the tiny problem of tests/test_gpu_mag_step.py: V = 50, H = 8, K = 4, S = 2, and
clip_norm = -1 as run_mag.sh sets it.

"exact" is held bit for bit to today's deterministic step (table_step=None) in every parameter, Adam tensor and loss, eager
and replayed.  "lazy" is held bit for bit to the numpy mirror of tests/optim_rows_cases.py fed the rows the step's own
backward left in its RowGrad; rows no batch touched keep their first bits.  "lazy" is not the reference's dense Adam."""
import numpy as np
import pytest
import torch

import optim_cases as oc
import optim_rows_cases as rc
import step_cases as sc
from test_gpu_mag_step import (BASE_SEED, BATCH, C, CONF, H, K, LAM, LR, N, N_TRAIN, N_UNLABEL, P_NODE, S, TEM, UNLABEL_BATCH, V, WARMUP,
                               _assert_twins, _same, selection, world)

pytestmark = pytest.mark.gpu


def mag_step(capture, table_step, nlayers=2, max_entries=None, clip_norm=-1.0, weight_decay=5e-4):
    """(MagTrainStep, model, optimizer) in deterministic mode over the shared problem, from the same initial state every time."""
    from grand_plus_amd import ClipAdam, MagTrainStep, StepState, mag_trained_parameters
    from grand_plus_amd.mlp import MagMLP
    from grand_plus_amd.rows import RowMatrix
    seeds, col, val, filled, attrs, labels, _longest = world()
    row = torch.from_numpy(np.repeat(seeds, K).astype(np.int32))
    rm = RowMatrix(seeds, K, row.cuda(), col.cuda(), val.cuda(), filled.cuda(), N)
    torch.manual_seed(7)
    m = MagMLP(V, C, H, nlayers, True, 0.0, 0.5, True).cuda().train()
    opt = ClipAdam(mag_trained_parameters(m), lr=LR, betas=oc.BETAS, eps=oc.EPS, weight_decay=weight_decay, clip_norm=clip_norm,
                   capturable=True, state=StepState("cuda"))
    kw = {} if table_step is None else dict(table_step=table_step)             # None: the call of the parent commit, word for word
    ts = MagTrainStep(m, opt, rm, *(a.cuda() for a in attrs), labels.cuda(), seeds[:N_TRAIN], seeds[N_TRAIN:], samples=S,
                      dropnode_rate=P_NODE, lam=LAM, warmup=WARMUP, tem=TEM, conf=CONF, kind="l2", seed=BASE_SEED, capture=capture,
                      deterministic=True, max_entries=max_entries, **kw)
    return ts, m, opt


def _poison(ts):
    ts.row_grad.values.fill_(float("nan"))


@pytest.mark.parametrize("capture", [False, True], ids=["eager", "replayed"])
def test_three_exact_steps_equal_todays_deterministic_step_bit_for_bit(capture):
    new, nm, no = mag_step(capture, "exact")
    old, om, oo = mag_step(capture, None)
    assert new.row_grad is not None and old.row_grad is None and new.row_grad.values.shape == (V, H)
    values_at = new.row_grad.values.data_ptr()
    for t in range(1, 4):
        sel = selection(t)
        _poison(new)                                                            # what the last step left in `values` is never read
        _assert_twins((new.step(*sel), nm, no), (old.step(*sel), om, oo), f"step {t}")
        assert nm.embeds.weight.grad is None and om.embeds.weight.grad is not None
        assert new.row_grad.filled() and new.row_grad.keys.dtype == torch.int64 and new.row_grad.n_sorted == new._max_entries(7)
    assert new.row_grad.values.data_ptr() == values_at                          # one buffer, every step and every graph
    touched = rc.touched(new.row_grad.keys.cpu().numpy(), V)
    assert touched.any() and not touched.all()
    assert bool(torch.isnan(new.row_grad.values[torch.from_numpy(~touched).cuda()]).all())      # the poison is still there
    assert bool(torch.isfinite(new.row_grad.values[torch.from_numpy(touched).cuda()]).all())
    assert (new._shapes.get((7, 3)) is not None) == capture
    new.check_entries_flag()
    assert set(no.state[nm.embeds.weight]) == {"step", "exp_avg", "exp_avg_sq"} and no.state[nm.embeds.weight]["exp_avg"].shape == (V, H)


def test_a_replayed_exact_step_waits_for_nothing():
    new, nm, no = mag_step(True, "exact")
    old, om, oo = mag_step(False, None)
    for t in range(1, 4):
        sel = selection(t)
        new.step(*sel), old.step(*sel)
    sel = selection(4)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = tuple(x.clone() for x in new.step(*sel))
    finally:
        torch.cuda.set_sync_debug_mode(0)
    want = old.step(*sel)
    for name, x, y in zip(want._fields, got, want):
        assert _same(x, y), f"step 4: {name} differs"
    _assert_twins((want, nm, no), (want, om, oo), "step 4")


def test_exact_step_sampled_gets_a_graph_per_shape_over_one_row_grad():
    """Three epochs of 3 + 3 + 1 labelled nodes: two batch shapes, two graphs, one RowGrad."""
    from grand_plus_amd import Sampler
    from grand_plus_amd._common import step_seed
    s = Sampler(N_TRAIN, N_UNLABEL, BATCH, UNLABEL_BATCH, 11)
    got, gm, go = mag_step(True, "exact")
    ref, rm_, ro = mag_step(False, None)
    for t in range(1, 10):
        a = got.step_sampled(s, t)
        b = ref.step(*s.selection(t, step_seed(BASE_SEED, t)))
        _assert_twins((a, gm, go), (b, rm_, ro), f"step {t}")
    assert len(got._sampled) == 2 and all(v is not None for v in got._sampled.values())
    got.check_selection_flag()
    got.check_entries_flag()


def test_exact_with_one_layer_where_the_table_is_the_only_parameter():
    new, nm, no = mag_step(True, "exact", nlayers=1)
    old, om, oo = mag_step(True, None, nlayers=1)
    assert not len(nm.fcs) and len(no.param_groups[0]["params"]) == 1
    for t in range(1, 4):
        sel = selection(t)
        _assert_twins((new.step(*sel), nm, no), (old.step(*sel), om, oo), f"one layer, step {t}")
    assert new._shapes[(7, 3)] is not None


def _dense_grads(ts, m, opt):
    """The gradients the step just taken gave every parameter of the optimiser, dense, on the CPU: `.grad` (the next step's
    zero_grad has not run yet), and for a table stepped from its RowGrad the zero-filled tensor that holds the touched rows."""
    out = []
    for p in (q for g in opt.param_groups for q in g["params"]):
        if p.grad is not None:
            out.append(p.grad.detach().cpu().clone())
        else:
            assert p is m.embeds.weight and ts.row_grad is not None
            out.append(torch.from_numpy(rc.dense_gradient(ts.row_grad.values.cpu().numpy(), ts.row_grad.keys.cpu().numpy())))
    return out


@pytest.mark.parametrize("nlayers", [2, 1], ids=["two-layers", "one-layer"])
def test_exact_with_clipping_on_the_norm_and_the_bound(nlayers):
    """With clipping on the two paths cut the norm's partial sums differently, so the coefficient may differ in its last
    bits, and in the two-layer model it reaches the dense groups' update as well.  Three eager steps with clip_norm = 0.1.
    The references are tests/optim_cases.py's: torch's clip_grad_norm_ + Adam(foreach=False) on the CPU in float64 and in
    float32, both fed the gradient sequence that the step under test produced itself (the table's rows as the zero-filled
    dense tensor), from the same initial parameters.  Every parameter and Adam tensor of the model is held to
    test_gpu_optim.py's bound, 4 max|torch32 - ref64| + 2^-23 max|ref64|; the norm of every step to 2^-23 of float64's;
    and at the first step, where both start from one state, to 2^-23 of today's dense step's norm."""
    new, nm, no = mag_step(False, "exact", nlayers=nlayers, clip_norm=0.1)
    old, om, oo = mag_step(False, None, nlayers=nlayers, clip_norm=0.1)
    params = [p for g in no.param_groups for p in g["params"]]
    assert (len(params) == 1) == (nlayers == 1) and params[0] is nm.embeds.weight
    init = [p.detach().cpu().clone() for p in params]
    seq, norms = [], []
    for t in range(1, 4):
        sel = selection(t)
        _poison(new)
        a = new.step(*sel)
        seq.append(_dense_grads(new, nm, no))
        norms.append(float(a.grad_norm))
        if t == 1:
            b = old.step(*sel)
            nb = float(b.grad_norm)
            print(f"nlayers {nlayers}: norm rows {norms[0]!r} dense {nb!r}")
            assert nb > 0.1 and abs(norms[0] - nb) <= 2.0 ** -23 * nb           # clipping is active
            assert _same(a.loss, b.loss)
            for x, y in zip(seq[0], _dense_grads(old, om, oo)):
                assert _same(x, y)                                              # one state, one gradient
    assert nm.embeds.weight.grad is None
    hyper = dict(lr=LR, weight_decay=5e-4, clip=0.1)
    r64, t32 = oc.torch_run(init, seq, hyper, torch.float64), oc.torch_run(init, seq, hyper, torch.float32)
    for got, ref in zip(norms, r64["norm"]):
        assert abs(got - float(ref)) <= 2.0 ** -23 * float(ref), (got, float(ref))
    ours = {"param": params, "exp_avg": [no.state[p]["exp_avg"] for p in params],
            "exp_avg_sq": [no.state[p]["exp_avg_sq"] for p in params]}
    oc.error_ratios(ours, t32, r64, f"table-step exact, clip on, nlayers {nlayers}")


def _lazy_run(capture, steps=3):
    """`steps` lazy steps; after each one the table, its moments, the RowGrad's keys and rows and the device's corrections."""
    ts, m, opt = mag_step(capture, "lazy", weight_decay=0.0)
    w = m.embeds.weight
    trace = [(w.detach().cpu().numpy().copy(), None, None, None, None, None)]
    results = []
    for t in range(1, steps + 1):
        _poison(ts)
        r = ts.step(*selection(t))
        results.append(tuple(x.clone() for x in r))
        img = ts.state.read()
        trace.append((w.detach().cpu().numpy().copy(), opt.state[w]["exp_avg"].cpu().numpy().copy(),
                      opt.state[w]["exp_avg_sq"].cpu().numpy().copy(), ts.row_grad.keys.cpu().numpy().copy(),
                      ts.row_grad.values.cpu().numpy().copy(), (img.step_size[0], img.rsqrt_bc2[0])))
    assert w.grad is None
    return ts, m, opt, trace, results


def test_three_lazy_steps_are_the_mirror_on_the_steps_own_rows_eager_and_replayed():
    ts, m, opt, trace, results = _lazy_run(True)
    _e_ts, em, eo, e_trace, e_results = _lazy_run(False)
    assert ts._shapes[(7, 3)] is not None
    for t, (ra, rb) in enumerate(zip(results, e_results), 1):
        for name, x, y in zip(("loss", "sup", "con", "n_conf", "n_correct", "grad_norm"), ra, rb):
            assert _same(x, y), f"lazy step {t}: {name} differs eager and replayed"
    for i, (x, y) in enumerate(zip(sc.snapshot(m, opt), sc.snapshot(em, eo))):
        assert _same(x, y), f"lazy: tensor {i} of the snapshot differs eager and replayed"
    p, mm, vv = trace[0][0], np.zeros((V, H), np.float32), np.zeros((V, H), np.float32)
    first = p.copy()
    ever = np.zeros(V, bool)
    for t in range(1, 4):
        got_p, got_m, got_v, keys, dW, (step_size, rsqrt_bc2) = trace[t]
        touched = rc.touched(keys, V)
        assert touched.any() and not touched.all() and np.isnan(dW[~touched]).all() and np.isfinite(dW[touched]).all()
        p, mm, vv, _ = rc.mirror_step("lazy", p, mm, vv, dW, keys, lr=LR, betas=oc.BETAS, eps=oc.EPS, weight_decay=0.0, clip=-1.0,
                                      step_size=step_size, rsqrt_bc2=rsqrt_bc2, dtype=np.float32)
        for name, got, want in (("param", got_p, p), ("exp_avg", got_m, mm), ("exp_avg_sq", got_v, vv)):
            assert rc.same_bits(got, want), f"lazy step {t}: {name} is not the mirror's"
        ever |= touched
    assert not ever.all()
    assert rc.same_bits(trace[3][0][~ever], first[~ever])                       # a row no batch touched never moved
    assert not trace[3][1][~ever].any() and not trace[3][2][~ever].any()         # nor did its moments
    assert not rc.same_bits(trace[3][0][ever], first[ever])
    # dense Adam is another trajectory: with today's step an untouched row moves under weight decay alone, and without it
    # stays only while its moments are still zero; the lazy table differs from the exact one from the second step on
    ex, xm, xo = mag_step(False, "exact", weight_decay=0.0)
    for t in range(1, 4):
        ex.step(*selection(t))
    assert not _same(xm.embeds.weight, m.embeds.weight)


def test_lazy_refuses_a_decayed_table_and_a_tight_max_entries_still_sets_the_flag():
    with pytest.raises(ValueError, match="'lazy' takes weight_decay = 0"):
        mag_step(True, "lazy", weight_decay=5e-4)
    for mode, wd in (("exact", 5e-4), ("lazy", 0.0)):
        ts, _m, _o = mag_step(True, mode, max_entries=1, weight_decay=wd)
        for t in range(1, 4):                                                    # eager, captured, replayed
            ts.step(*selection(t))
        assert ts.row_grad.n_sorted == 1
        with pytest.raises(RuntimeError, match="more entries than max_entries = 1"):
            ts.check_entries_flag()
