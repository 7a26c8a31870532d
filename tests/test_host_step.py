"""CPU tests of the device-resident step state: the seed and weight mirrors follow their formulas, the C
entry points return their error codes before any GPU work, and ClipAdam(capturable=True) and TrainStep refuse what they
cannot run before any device call."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import abi_header
from grand_plus_amd import _common, _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(16)
M = 2 ** 64 - 1


def _fmix(x):
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
    return x ^ (x >> 31)


def test_step_seed_is_the_formula_of_the_header_with_known_answers():
    text, _ = abi_header.read("grandplus_step.h")
    m = re.search(r"#define GP_STEP_MUL (0x[0-9A-F]{16})ull\n", text)
    assert m and "mix(base_seed ^ tick * GP_STEP_MUL)" in text
    mul = int(m.group(1), 16)
    assert mul % 2 == 1
    for unit in ("gp_common.hpp", "dropnode.hpp", "mag_prop.hip", "mlp.hip"):       # a new constant: no other derivation uses it
        assert m.group(1) not in open(os.path.join(ROOT, "grand_plus_amd", "csrc", unit)).read()
    hip = open(os.path.join(ROOT, "grand_plus_amd", "csrc", "step_state.hip")).read()
    assert "GP_STEP_MUL" in hip and m.group(1) not in hip                             # the unit takes it from the header
    for name in ("fmix64", "mix64", "sample_seed", "layer_sample_seed", "keep_scale", "inv_keep"):
        assert not re.search(r"\b%s\s*\([^;{]*\)\s*\{" % name, hip), f"step_state.hip restates {name}"
    for name in ("mix64", "sample_seed", "layer_sample_seed", "keep_scale", "inv_keep"):
        assert re.search(r"\b%s\(" % name, hip), f"step_state.hip does not call {name}"
    for base, t in [(0, 1), (0x5EED, 2), (M, 300), (123456789, 2 ** 40)]:
        want = _fmix(((base ^ (t * mul & M)) + 0x9E3779B97F4A7C15) & M)
        assert _common.step_seed(base, t) == want and 0 <= want <= M
        assert _common.step_seed(base, t) != _common.step_seed(base, t + 1)
        assert _common.step_seed(base, t) != _common.sample_seed(base, t)
    # values worked out once from the formula: a change of it shows here
    assert _common.step_seed(0, 1) == 0xE65C8202A38ACA67
    assert _common.step_seed(0x5EED, 2) == 0x2FA64E2775DD0E54
    assert _common.step_seed(M, 300) == 0xB65AB3BB152E7664
    from grand_plus_amd import step
    assert step.step_seed is _common.step_seed
    assert len(re.findall(r"^def step_seed", open(os.path.join(ROOT, "grand_plus_amd", "_common.py")).read(), flags=re.M)) == 1


@pytest.mark.parametrize("lam,warmup", [(1.0, 100), (0.7, 5), (1.5, 7), (0.0, 10), (1.0, 1), (0.3, 1)])
def test_the_weight_schedule_in_float32(lam, warmup):
    """min(lam, lam * num_batch / warmup) of model.py:329 with num_batch = t - 1: 0 at the first step, lam from step
    warmup + 1 on, never above lam, and the float32 of the double in between."""
    from grand_plus_amd.step import step_weight
    ws = [step_weight(lam, warmup, t) for t in range(1, warmup + 4)]
    assert all(isinstance(w, np.float32) for w in ws)
    assert ws[0] == 0.0
    for t, w in enumerate(ws, start=1):
        num_batch = t - 1
        assert w == np.float32(min(lam, lam * num_batch / warmup))               # the reference's expression, rounded once
        assert w <= np.float32(lam)
    assert all(w == np.float32(lam) for w in ws[warmup:])                        # t >= warmup + 1
    assert all(a <= b for a, b in zip(ws, ws[1:]))
    if lam == 0.0:
        assert all(w == 0.0 for w in ws)
    if warmup == 1:
        assert ws[1] == np.float32(lam)


def _advance(st=P, base=1, lam=1.0, warmup=10.0, n=1, lr=(1e-2,), b1=(0.9,), b2=(0.999,)):
    arr = lambda v: (ctypes.c_double * max(len(v), 1))(*v) if v is not None else None   # noqa: E731
    return _native.lib().gp_step_advance(0, st, base, lam, warmup, n, arr(lr), arr(b1), arr(b2), None)


def _seg(**kw):
    d = dict(keep=16, keep_stride=64, batch_rows=16, filled=16, kind=0, n_samples=2, n_batch=4, K=8, width=0, layer=0, p=0.5, pad=0)
    d.update(kw)
    return _native.GpStepSegment(**d)


def _masks(segs, st=P, n=None):
    tab = (_native.GpStepSegment * max(len(segs), 1))(*segs)
    return _native.lib().gp_step_masks(0, st, tab if segs is not None else None, len(segs) if n is None else n, None)


def _layer(**kw):
    return _seg(**{**dict(kind=1, batch_rows=None, filled=None, K=0, width=5), **kw})


def test_the_entries_return_their_error_codes_before_any_gpu_work():
    """No device pointer here is real: every call has to stop at its argument checks."""
    E, N, OK = _native.GP_ERR_INVALID_ARG, _native.GP_ERR_NULL, _native.GP_OK
    nan, inf = float("nan"), float("inf")
    assert _advance(n=-1) == E and _advance(n=9) == E
    assert "gp_step_advance" in _native.lib().gp_last_error().decode()
    assert _advance(lam=nan) == E and _advance(lam=inf) == E
    assert _advance(warmup=0.0) == E and _advance(warmup=-1.0) == E and _advance(warmup=nan) == E and _advance(warmup=inf) == E
    assert _advance(lr=(nan,)) == E and _advance(b1=(1.0,)) == E and _advance(b1=(-0.1,)) == E and _advance(b2=(1.0,)) == E
    assert _advance(b2=(nan,)) == E
    assert _advance(st=None) == N and _advance(lr=None) == N and _advance(b1=None) == N and _advance(b2=None) == N

    assert _masks([_seg()], n=-1) == E and _masks([_seg()] * 10) == E
    assert "gp_step_masks" in _native.lib().gp_last_error().decode()
    assert _masks([_seg(kind=2)]) == E and _masks([_seg(kind=-1)]) == E
    assert _masks([_seg(n_samples=0)]) == E and _masks([_seg(n_samples=17)]) == E and _masks([_seg(n_batch=-1)]) == E
    assert _masks([_seg(p=-0.1)]) == E and _masks([_seg(p=1.5)]) == E and _masks([_seg(p=nan)]) == E
    assert _masks([_seg(K=0)]) == E and _masks([_seg(K=_native.GP_MAX_K + 1)]) == E and _masks([_seg(keep_stride=-1)]) == E
    assert _masks([_layer(width=0)]) == E and _masks([_layer(layer=-1)]) == E and _masks([_layer(layer=8)]) == E
    assert _masks([_seg()], st=None) == N and _masks([_seg(keep=None)]) == N and _masks([_seg(batch_rows=None)]) == N
    assert _masks([_layer(keep=None)]) == N
    assert _native.lib().gp_step_masks(0, P, None, 1, None) == N
    # nothing to do: GP_OK with nothing launched -- no segment, p = 0 (nothing is drawn), an empty batch
    assert _masks([]) == OK
    assert _masks([_seg(p=0.0), _layer(p=0.0)]) == OK and _masks([_seg(n_batch=0), _layer(n_batch=0)]) == OK
    assert _masks([_seg(p=0.0), _seg(kind=3)]) == E                          # ... but every segment is still checked

    t = _native.GpOptimTensor(param=16, grad=16, exp_avg=16, exp_avg_sq=16, numel=4)
    tab = (_native.GpOptimTensor * 1)(t)

    def dev(flags=0, ss=P, bc=P, ws=P, norm=P, n=1, max_norm=0.1):
        return _native.lib().gp_clip_adam_step_dev(0, tab, n, flags, max_norm, 1e-2, 0.9, 0.999, 1e-8, 0.0, ss, bc, ws, norm, None)

    assert dev(n=-1) == E and dev(flags=8) == E and dev(max_norm=nan) == E
    assert "gp_clip_adam_step_dev" in _native.lib().gp_last_error().decode()
    assert dev(flags=_native.GP_OPTIM_NORM_ONLY | _native.GP_OPTIM_NORM_READY) == E
    assert dev(ss=None) == N and dev(bc=None) == N and dev(ws=None) == N and dev(norm=None) == N


# ---- ClipAdam(capturable=True): every tensor is on the CPU and the native library raises if it is reached
def _params(n=3, grads=True):
    ps = [torch.nn.Parameter(torch.zeros(4)) for _ in range(n)]
    for p in ps:
        p.grad = torch.ones(4) if grads else None
    return ps


class _FakeState:
    """Stands in for a StepState where no device exists: it records the tick it is given and nothing else."""
    tick = None

    def set_tick(self, t):
        self.tick = t


def test_capturable_clipadam_refuses_before_any_launch(monkeypatch):
    from grand_plus_amd import ClipAdam
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the native library was reached"))
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(lr=torch.tensor(1e-3))):
        with pytest.raises(ValueError):
            ClipAdam(_params(), capturable=True, state=_FakeState(), **kw)
    with pytest.raises(TypeError, match="missing its StepState"):               # the state is a required argument of capturable
        ClipAdam(_params(), capturable=True)
    with pytest.raises(ValueError, match="state= is the step count"):
        ClipAdam(_params(), state=_FakeState())
    assert ClipAdam(_params()).capturable is False and ClipAdam(_params()).step_state is None
    st = _FakeState()
    opt = ClipAdam(_params(), capturable=True, state=st)
    assert opt.capturable is True and opt.step_state is st

    ps = _params()
    ps[1].grad = None
    opt = ClipAdam(ps, capturable=True, state=_FakeState())
    with pytest.raises(ValueError, match="a parameter has no gradient"):
        opt.step()
    assert len(opt.state) == 0

    opt = ClipAdam([{"params": [p]} for p in _params(9)], capturable=True, state=_FakeState())
    with pytest.raises(ValueError, match="at most 8 parameter groups, got 9"):
        opt.step()

    ps = _params()
    opt = ClipAdam(ps, capturable=True, state=_FakeState())
    for p, t in zip(ps, (3, 3, 4)):
        opt.state[p] = {"step": t, "exp_avg": torch.zeros(4), "exp_avg_sq": torch.zeros(4)}
    with pytest.raises(ValueError, match=re.escape("the loaded values are [3, 4]")):
        opt.step()
    assert [opt.state[p]["step"] for p in ps] == [3, 3, 4]

    # a checkpoint whose step counts differ is refused at load; one that leaves a parameter without state at the step
    adam = torch.optim.Adam(ps)
    for p, t in zip(ps, (2.0, 2.0, 5.0)):
        adam.state[p] = {"step": torch.tensor(t), "exp_avg": torch.zeros(4), "exp_avg_sq": torch.zeros(4)}
    st = _FakeState()
    opt = ClipAdam(ps, capturable=True, state=st)
    with pytest.raises(ValueError, match=re.escape("the checkpoint holds [2, 5]")):
        opt.load_state_dict(adam.state_dict())
    assert len(opt.state) == 0 and st.tick is None
    del adam.state[ps[2]]
    opt.load_state_dict(adam.state_dict())
    assert st.tick == 2
    with pytest.raises(ValueError, match=re.escape("the loaded values are [0, 2]")):
        opt.step()


def test_the_default_clipadam_reaches_none_of_the_new_code(monkeypatch):
    from grand_plus_amd import ClipAdam, optim

    def boom(*_a, **_k):
        raise AssertionError("capturable=False reached the capturable path")

    monkeypatch.setattr(optim, "_call_dev", boom)
    monkeypatch.setattr(ClipAdam, "_check_capturable", boom)
    monkeypatch.setattr(ClipAdam, "_step_capturable", boom)
    opt = ClipAdam(_params())
    with pytest.raises(TypeError, match="must be a CUDA tensor"):                # the last host check of before
        opt.step()
    sd = opt.state_dict()
    opt.load_state_dict(sd)
    assert all(g.get("capturable", False) is False for g in sd["param_groups"])


# ---- TrainStep
def _rows(n_nodes=12, S_rows=6, K=4):
    from grand_plus_amd.rows import RowMatrix
    z = torch.zeros(S_rows * K, dtype=torch.int32)
    return RowMatrix(np.arange(S_rows), K, z, z, torch.zeros(S_rows * K, dtype=torch.float64),
                     torch.full((S_rows,), K, dtype=torch.int32), n_nodes)


def _train_step(model=None, opt=None, rows=None, features=None, **kw):
    from grand_plus_amd import ClipAdam, TrainStep
    from grand_plus_amd.mlp import GrandPlusMLP
    from grand_plus_amd.step import trained_parameters
    model = GrandPlusMLP(5, 3, 4, 2, True, 0.5, 0.5, True).train() if model is None else model
    opt = ClipAdam(trained_parameters(model), capturable=True, state=_FakeState()) if opt is None else opt
    args = dict(samples=2, dropnode_rate=0.5, lam=1.0, warmup=10, tem=0.5, seed=1)
    args.update(kw)
    return TrainStep(model, opt, _rows() if rows is None else rows, torch.zeros((12, 5)) if features is None else features,
                     torch.zeros(12, dtype=torch.int64), [0, 1, 2], [3, 4, 5], **args)


def test_train_step_refuses_before_any_device_call(monkeypatch):
    from grand_plus_amd import ClipAdam, TrainStep
    from grand_plus_amd.mlp import GrandPlusMLP, MagMLP
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the native library was reached"))
    mag = MagMLP(9, 3, 4, 2, True, 0.5, 0.5, True).train()
    with pytest.raises(ValueError, match="takes a GrandPlusMLP"):
        _train_step(model=mag, opt=ClipAdam(mag.parameters(), capturable=True, state=_FakeState()))
    model = GrandPlusMLP(5, 3, 4, 2, True, 0.5, 0.5, True).train()
    with pytest.raises(ValueError, match=re.escape("ClipAdam(capturable=True)")):
        _train_step(model=model, opt=ClipAdam(model.parameters()))
    with pytest.raises(ValueError, match=re.escape("ClipAdam(capturable=True)")):
        _train_step(model=model, opt=torch.optim.Adam(model.parameters()))
    with pytest.raises(ValueError, match="must not require grad"):
        _train_step(features=torch.zeros((12, 5), requires_grad=True))
    with pytest.raises(ValueError, match="rows must be a RowMatrix"):
        _train_step(rows=object())
    for kw, msg in ((dict(samples=0), "samples"), (dict(samples=17), "samples"), (dict(samples=2.0), "samples"),
                    (dict(dropnode_rate=1.5), "dropnode_rate"), (dict(kind="mse"), "kind"), (dict(tem=0.0), "tem")):
        with pytest.raises(ValueError, match=msg):
            _train_step(**kw)
    with pytest.raises(ValueError, match="no CPU fallback"):                     # everything else passes: only the device is missing
        _train_step()
    # eval mode: step() raises before it looks at its arguments or at the device
    ts = object.__new__(TrainStep)
    ts.model = model.eval()
    with pytest.raises(RuntimeError, match="train mode"):
        ts.step(None, None)
    assert not model.training


def test_selections_are_range_checked_on_the_host():
    from grand_plus_amd.step import _selection
    assert _selection(np.array([0, 4, 2]), 5, "sel").tolist() == [0, 4, 2]
    assert _selection(torch.tensor([1, 0], dtype=torch.int32), 2, "sel").dtype == np.int64
    assert _selection([], 0, "sel").size == 0
    for bad in ([5], [-1], [0, 1, 7], torch.tensor([3, -2])):
        with pytest.raises(IndexError, match=r"sel holds an index outside \[0, 5\)"):
            _selection(bad, 5, "sel")


def test_the_names_are_reachable_from_the_package_and_stay_out_of_all():
    import grand_plus_amd
    from grand_plus_amd import step
    assert grand_plus_amd.TrainStep is step.TrainStep and grand_plus_amd.StepState is step.StepState
    assert "TrainStep" not in grand_plus_amd.__all__ and "StepState" not in grand_plus_amd.__all__
    assert step.MAX_GRAPHS == 4
    assert step.StepResult._fields == ("loss", "sup", "con", "n_conf", "n_correct", "grad_norm")
