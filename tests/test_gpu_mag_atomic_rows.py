"""MAG's atomic table gradient as a row list: `mag_prop_rows(..., row_grad=BitmapRowGrad, deterministic=False,
max_entries=...)` on every case of tests/mag_cases.py against the float64 reference under the bound tests/test_gpu_mag_rows.py
holds the atomic backward to, and `MagTrainStep(table_step=..., row_list="bitmap", deterministic=False)` at the tiny problem
of tests/test_gpu_mag_step.py (V = 50, H = 8): the key list against the deterministic step's, the table and its moments
against the numpy mirror ("lazy") and the dense kernel ("exact") driven by the step's own rows."""
import numpy as np
import pytest
import torch

import mag_cases as mc
import optim_cases as oc
import optim_rows_cases as rc
import row_mark_cases as rm
from test_gpu_mag_rows import _cuda, _run, _same
from test_gpu_mag_step import (BASE_SEED, BATCH, C, CONF, H, K, LAM, LR, N, N_TRAIN, N_UNLABEL, P_NODE, S, TEM, UNLABEL_BATCH, V, WARMUP,
                               selection, world)

pytestmark = pytest.mark.gpu


def _capacity(c):
    P = c["P"]
    B = P.S_rows if c["batch"] is None else c["batch"].numel()
    return max(1, B * P.K * P.longest)


# ---- the op
@pytest.mark.parametrize("name", list(mc.CASES))
def test_the_row_list_gradient_matches_float64_and_the_poison_survives(name):
    from grand_plus_amd import BitmapRowGrad
    c = mc.case(name)
    P = c["P"]
    _out64, _terms, dW64, dW_terms = c["ref"]
    W = P.W.cuda().requires_grad_(True)
    rg = BitmapRowGrad(W)
    rg.values.fill_(float("nan"))
    M = _capacity(c)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = _run(c, W=W, keep=_cuda(c["keep"]), row_grad=rg, deterministic=False, max_entries=M, overflow=flag)
    assert _same(out.detach(), _run(c, keep=_cuda(c["keep"])))                    # the forward is untouched
    assert not rg.filled()
    (out * c["G"].cuda()).sum().backward()
    assert W.grad is None and rg.filled() and int(flag.item()) == 0
    keys, values = rg.keys.cpu().numpy(), rg.values.cpu().numpy()
    marked = rm.marked_rows(P, None if c["batch"] is None else c["batch"].tolist())
    assert keys.dtype == np.int64 and np.array_equal(keys, rm.list_keys(marked, P.V, min(P.V, M)))
    assert int(rg.count.item()) == len(marked) and not bool(rg.bitmap.any())       # the bitmap is ready for the next call
    touched = rc.touched(keys, P.V)
    assert np.isnan(values[~touched]).all() and np.isfinite(values[touched]).all()
    dense = torch.from_numpy(rc.dense_gradient(values, keys))
    ratio = mc.close(dense, dW64, dW_terms, c["roundings"], f"{name} dW from the row list")
    print(f"[mag rows] {name}: {len(marked)} of {P.V} rows listed, dW error / bound {ratio:.3g}")
    assert not bool(dW64[torch.from_numpy(~touched)].any())                         # the list is a superset of the gradient's rows


def test_a_tight_capacity_sets_the_flag_and_lists_the_first_rows():
    from grand_plus_amd import BitmapRowGrad
    c = mc.case("h7_k5_s3")
    P = c["P"]
    marked = rm.marked_rows(P, c["batch"].tolist())
    W = P.W.cuda().requires_grad_(True)
    rg = BitmapRowGrad(W)
    for M, over in ((len(marked) - 1, True), (len(marked), False), (3, True)):
        rg.values.fill_(float("nan"))
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        out = _run(c, W=W, keep=_cuda(c["keep"]), row_grad=rg, deterministic=False, max_entries=M, overflow=flag)
        (out * c["G"].cuda()).sum().backward()
        assert int(flag.item()) == int(over) and rg.n_sorted == M and int(rg.count.item()) == len(marked)
        assert np.array_equal(rg.keys.cpu().numpy(), marked[:M]) and not bool(rg.bitmap.any())
        values = rg.values.cpu().numpy()
        mc.close(torch.from_numpy(values[marked[:M]]), c["ref"][2][marked[:M]], c["ref"][3][marked[:M]], c["roundings"], f"capacity {M}")


def test_forward_and_backward_wait_for_nothing():
    from grand_plus_amd import BitmapRowGrad
    c = mc.case("h64_k32_s2")
    W = c["P"].W.cuda().requires_grad_(True)
    rg = BitmapRowGrad(W)
    from grand_plus_amd import mag_prop_rows
    ops = c["P"].cuda()[1:] + (_cuda(c["batch"]),)                                  # every upload comes first
    kw = dict(c["kw"], keep=_cuda(c["keep"]), row_grad=rg, deterministic=False, max_entries=_capacity(c),
              overflow=torch.zeros(1, dtype=torch.int32, device="cuda"))
    G = c["G"].cuda()
    (mag_prop_rows(W, *ops, **kw) * G).sum().backward()                             # the library is loaded
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        (mag_prop_rows(W, *ops, **kw) * G).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert W.grad is None and rg.filled()


# ---- the step
def mag_step(capture, table_step, deterministic=False, max_entries=None, weight_decay=5e-4):
    """(MagTrainStep, model, optimizer) over the shared problem from the same initial state every time: the atomic backward
    with row_list="bitmap", or (deterministic=True) the deterministic step of DESIGN §7t beside it.  clip_norm = -1."""
    from grand_plus_amd import ClipAdam, MagTrainStep, StepState, mag_trained_parameters
    from grand_plus_amd.mlp import MagMLP
    from grand_plus_amd.rows import RowMatrix
    seeds, col, val, filled, attrs, labels, _longest = world()
    row = torch.from_numpy(np.repeat(seeds, K).astype(np.int32))
    rmx = RowMatrix(seeds, K, row.cuda(), col.cuda(), val.cuda(), filled.cuda(), N)
    torch.manual_seed(7)
    m = MagMLP(V, C, H, 2, True, 0.0, 0.5, True).cuda().train()
    opt = ClipAdam(mag_trained_parameters(m), lr=LR, betas=oc.BETAS, eps=oc.EPS, weight_decay=weight_decay, clip_norm=-1.0,
                   capturable=True, state=StepState("cuda"))
    kw = dict(deterministic=True) if deterministic else dict(deterministic=False, row_list="bitmap")
    ts = MagTrainStep(m, opt, rmx, *(a.cuda() for a in attrs), labels.cuda(), seeds[:N_TRAIN], seeds[N_TRAIN:], samples=S,
                      dropnode_rate=P_NODE, lam=LAM, warmup=WARMUP, tem=TEM, conf=CONF, kind="l2", seed=BASE_SEED, capture=capture,
                      max_entries=max_entries, table_step=table_step, **kw)
    return ts, m, opt


def _run_steps(capture, table_step, steps=3, **kw):
    """`steps` steps with `values` poisoned before each; per step the table and its moments before and after, the RowGrad's
    keys and rows, the device's corrections and the step's results."""
    from grand_plus_amd.optim_rows import BitmapRowGrad
    ts, m, opt = mag_step(capture, table_step, **kw)
    assert type(ts.row_grad) is BitmapRowGrad and ts.row_list == "bitmap"
    w = m.embeds.weight
    zero = np.zeros((V, H), np.float32)
    trace = []

    def table():
        st = opt.state.get(w, {})
        return (w.detach().cpu().numpy().copy(), st["exp_avg"].cpu().numpy().copy() if "exp_avg" in st else zero.copy(),
                st["exp_avg_sq"].cpu().numpy().copy() if "exp_avg_sq" in st else zero.copy())

    for t in range(1, steps + 1):
        before = table()
        ts.row_grad.values.fill_(float("nan"))
        r = tuple(x.clone() for x in ts.step(*selection(t)))
        img = ts.state.read()
        trace.append(dict(before=before, after=table(), keys=ts.row_grad.keys.cpu().numpy().copy(),
                          values=ts.row_grad.values.cpu().numpy().copy(), corr=(float(img.step_size[0]), float(img.rsqrt_bc2[0])),
                          result=r))
        assert not bool(ts.row_grad.bitmap.any())
    assert w.grad is None and (ts._shapes.get((7, 3)) is not None) == capture
    ts.check_entries_flag()
    return ts, trace


def _det_distinct_keys(steps=3):
    """The distinct in-range keys of the deterministic step's sorted key list, step by step (they depend on the selection
    alone, not on the weights)."""
    ts, _m, _o = mag_step(False, "exact", deterministic=True)
    out = []
    for t in range(1, steps + 1):
        ts.step(*selection(t))
        k = ts.row_grad.keys.cpu().numpy()
        out.append(np.unique(k[(k >= 0) & (k < V)]))
    return out


def _check_rows(step, t):
    keys, values = step["keys"], step["values"]
    touched = rc.touched(keys, V)
    assert touched.any() and not touched.all() and np.isnan(values[~touched]).all() and np.isfinite(values[touched]).all(), f"step {t}"
    return touched


def test_three_lazy_steps_are_the_mirror_on_the_steps_own_rows_eager_and_replayed():
    det = _det_distinct_keys()
    runs = {capture: _run_steps(capture, "lazy", weight_decay=0.0) for capture in (False, True)}
    for capture, (ts, trace) in runs.items():
        first = trace[0]["before"][0]
        ever = np.zeros(V, bool)
        for t, step in enumerate(trace, 1):
            touched = _check_rows(step, t)
            cap = min(V, ts._max_entries(BATCH + UNLABEL_BATCH))
            assert np.array_equal(step["keys"], rm.list_keys(det[t - 1], V, cap)), f"capture={capture} step {t}: not the det step's distinct keys"
            p, mm, vv = step["before"]
            p, mm, vv, _ = rc.mirror_step("lazy", p, mm, vv, step["values"], step["keys"], lr=LR, betas=oc.BETAS, eps=oc.EPS,
                                          weight_decay=0.0, clip=-1.0, step_size=step["corr"][0], rsqrt_bc2=step["corr"][1])
            for name, got, want, old in zip(("param", "exp_avg", "exp_avg_sq"), step["after"], (p, mm, vv), step["before"]):
                assert rc.same_bits(got, want), f"capture={capture} lazy step {t}: {name} is not the mirror's"
                assert rc.same_bits(got[~touched], old[~touched]), f"capture={capture} lazy step {t}: an untouched row of {name} moved"
            ever |= touched
        assert not ever.all() and rc.same_bits(trace[-1]["after"][0][~ever], first[~ever])
        assert not rc.same_bits(trace[-1]["after"][0][ever], first[ever])               # the table is trained
    for t, (a, b) in enumerate(zip(runs[False][1], runs[True][1]), 1):
        assert np.array_equal(a["keys"], b["keys"]), f"step {t}: the key list differs eager and replayed"


def _dense_table_step(before, dense, corr, weight_decay):
    """gp_clip_adam_step (the dense kernel) on the table alone from `before` with the zero-filled gradient `dense`."""
    from grand_plus_amd import optim
    Pp, M, Vv, Gg = (torch.from_numpy(x.copy()).cuda() for x in (*before, dense))
    ws, norm = optim._buffers(Pp.device)
    optim._call(Pp.device, Pp, [(Pp, Gg, M, Vv)], 0, ws, norm, max_norm=-1.0, lr=LR, betas=oc.BETAS, eps=oc.EPS,
                weight_decay=weight_decay, step_size=corr[0], rsqrt_bc2=corr[1])
    return Pp.cpu().numpy(), M.cpu().numpy(), Vv.cpu().numpy()


@pytest.mark.parametrize("capture", [False, True], ids=["eager", "replayed"])
def test_three_exact_steps_are_the_dense_kernel_on_the_steps_own_rows(capture):
    det = _det_distinct_keys()
    ts, trace = _run_steps(capture, "exact")
    for t, step in enumerate(trace, 1):
        touched = _check_rows(step, t)
        assert np.array_equal(step["keys"][:len(det[t - 1])], det[t - 1]) and (step["keys"][len(det[t - 1]):] == V).all()
        want = _dense_table_step(step["before"], rc.dense_gradient(step["values"], step["keys"]), step["corr"], 5e-4)
        for name, got, ref, old in zip(("param", "exp_avg", "exp_avg_sq"), step["after"], want, step["before"]):
            assert rc.same_bits(got, ref), f"exact step {t}: {name} is not the dense kernel's"
        assert not rc.same_bits(step["after"][0][~touched], step["before"][0][~touched])   # dense Adam moves an untouched row


def test_a_replayed_step_waits_for_nothing_and_its_first_loss_is_the_det_steps():
    ts, m, _o = mag_step(True, "lazy", weight_decay=0.0)
    det, _dm, _do = mag_step(False, "lazy", deterministic=True, weight_decay=0.0)
    a, b = ts.step(*selection(1)), det.step(*selection(1))
    assert _same(a.loss, b.loss)                                                    # one state, one forward
    for t in (2, 3):
        ts.step(*selection(t))
    sel = selection(4)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        r = ts.step(*sel)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert bool(torch.isfinite(r.loss)) and bool(torch.isfinite(m.embeds.weight).all())


def test_step_sampled_gets_a_graph_per_shape_over_one_bitmap_row_grad():
    """Three epochs of 3 + 3 + 1 labelled nodes: two batch shapes, two graphs, one BitmapRowGrad and one bitmap."""
    from grand_plus_amd import Sampler
    s = Sampler(N_TRAIN, N_UNLABEL, BATCH, UNLABEL_BATCH, 11)
    ts, m, opt = mag_step(True, "exact")
    rg, values_at, bitmap_at = ts.row_grad, ts.row_grad.values.data_ptr(), ts.row_grad.bitmap.data_ptr()
    w0 = m.embeds.weight.detach().clone()
    for t in range(1, 10):
        r = ts.step_sampled(s, t)
        assert bool(torch.isfinite(r.loss)), t
    assert len(ts._sampled) == 2 and all(v is not None for v in ts._sampled.values())
    assert ts.row_grad is rg and rg.values.data_ptr() == values_at and rg.bitmap.data_ptr() == bitmap_at
    assert not bool(rg.bitmap.any()) and 0 < int(rg.count.item()) < V
    assert bool(torch.isfinite(m.embeds.weight).all()) and not torch.equal(w0, m.embeds.weight) and m.embeds.weight.grad is None
    ts.check_selection_flag()
    ts.check_entries_flag()


def test_a_tight_max_entries_sets_the_flag():
    for mode, wd in (("exact", 5e-4), ("lazy", 0.0)):
        ts, _m, _o = mag_step(True, mode, max_entries=1, weight_decay=wd)
        for t in range(1, 4):                                                      # eager, captured, replayed
            ts.step(*selection(t))
        assert ts.row_grad.n_sorted == 1
        with pytest.raises(RuntimeError, match="more table rows than max_entries = 1"):
            ts.check_entries_flag()
