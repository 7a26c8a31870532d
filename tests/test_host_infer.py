"""CPU tests of the inference path: the C entry point returns its error codes before any GPU work, and
`infer` / `local_logits` refuse what they cannot run before any launch (there is no CPU fallback)."""
import ctypes
import re

import pytest
import torch

import infer_cases as ic
from grand_plus_amd import _native

P = ctypes.c_void_p(16)


def test_local_logits_is_importable_from_the_package():
    import grand_plus_amd
    from grand_plus_amd import local_logits
    assert local_logits.__module__ == "grand_plus_amd.evaluate" and "local_logits" not in grand_plus_amd.__all__


def _call(x=P, n=4, f_in=3, f_out=2, w=P, b=P, flags=0, g=P, be=P, rm=P, rv=P, eps=1e-5, out=P, ws=P):
    return _native.lib().gp_mlp_infer_block(0, x, n, f_in, f_out, w, b, flags, g, be, rm, rv, eps, out, ws, None)


def test_the_entry_returns_its_error_codes_before_any_gpu_work():
    """No device pointer here is real: every call has to stop at its argument checks."""
    E, N, OK = _native.GP_ERR_INVALID_ARG, _native.GP_ERR_NULL, _native.GP_OK
    R, NORM, BN, TR = _native.GP_MLP_RELU, _native.GP_MLP_NORM, _native.GP_MLP_BN, _native.GP_MLP_TRAINING
    assert _call(n=-1) == E
    assert "gp_mlp_infer_block" in _native.lib().gp_last_error().decode()
    assert _call(f_in=0) == E and _call(f_out=0) == E and _call(f_in=-3) == E
    assert _call(flags=TR) == E and _call(flags=R | NORM | BN | TR) == E and _call(flags=16) == E and _call(flags=-1) == E
    assert _call(n=2 ** 40 + 1) == E and _call(f_out=2 ** 22 + 1) == E and _call(f_in=2 ** 31 - 1, f_out=2 ** 22) == E
    assert _call(flags=BN, eps=0.0) == E and _call(flags=BN, eps=-1.0) == E and _call(flags=BN, eps=float("nan")) == E
    assert _call(x=None) == N and _call(w=None) == N and _call(out=None) == N
    assert _call(flags=BN, rm=None) == N and _call(flags=BN, rv=None) == N
    assert _call(flags=NORM, ws=None) == N and _call(flags=BN, ws=None) == N and _call(flags=R | NORM | BN, ws=None) == N
    # nothing to do: GP_OK, nothing launched, the pointers not looked at
    assert _call(n=0) == OK and _call(n=0, x=None, out=None, ws=None, flags=R | NORM | BN) == OK
    assert _call(n=0, flags=TR) == E and _call(n=0, f_in=0) == E


def _model(bn=True, norm=True):
    from grand_plus_amd.mlp import GrandPlusMLP
    return GrandPlusMLP(5, 3, 4, 2, bn, 0.5, 0.5, norm).train()


def _no_stats():
    m = _model()
    m.bns[1] = torch.nn.BatchNorm1d(4, track_running_stats=False)
    return m


# every tensor here is on the CPU: shape, dtype, layout and size are refused before the device is looked at
@pytest.mark.parametrize("make,kw,msg", [
    (_model, dict(X=torch.zeros((2, 6, 5))), "infer takes X [B, F]"),
    (_model, dict(X=torch.zeros(5)), "infer takes X [B, F]"),
    (_model, dict(X=torch.zeros((6, 5), dtype=torch.float64)), "X must be float32"),
    (_model, dict(X=torch.zeros((6, 5), dtype=torch.float16)), "X must be float32"),
    (_model, dict(X=torch.zeros((5, 6)).t()), "X must be contiguous"),
    (_model, dict(X=None), "X must be a tensor"),
    (_model, dict(X=torch.zeros((6, 4))), "the layer takes 5 features, its input has 4"),
    (_model, dict(out=torch.zeros((6, 4))), "out must be [B, C] = (6, 3)"),
    (_model, dict(out=torch.zeros((5, 3))), "out must be [B, C] = (6, 3)"),
    (_model, dict(out=torch.zeros((6, 3), dtype=torch.float64)), "out must be a contiguous float32"),
    (_model, dict(out=torch.zeros((3, 6)).t()), "out must be a contiguous float32"),
    (_model, dict(out=torch.zeros((6, 3), device="meta")), "out must be on X's device"),
    (_model, dict(batch_size=0), "batch_size must be >= 1"),
    (_model, dict(batch_size=-5), "batch_size must be >= 1"),
    (_no_stats, dict(), "without running statistics"),
    (_model, dict(), "no CPU fallback"),
    (_model, dict(out=torch.zeros((6, 3)), batch_size=2), "no CPU fallback"),
    (lambda: _model(False, False), dict(X=torch.zeros((0, 5))), "no CPU fallback"),
])
def test_infer_refuses_before_any_launch(make, kw, msg, monkeypatch):
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the native library was reached"))
    model = make()
    args = dict(X=torch.zeros((6, 5)))
    args.update(kw)
    with pytest.raises(ValueError, match=re.escape(msg)):
        model.infer(args.pop("X"), **args)
    assert model.training                                    # nothing touched the model


def test_local_logits_and_predict_refuse_before_any_launch(monkeypatch):
    from grand_plus_amd import local_logits, predict
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the native library was reached"))
    with pytest.raises(TypeError, match="model must be"):
        local_logits(lambda x: x, torch.zeros((6, 5)))
    with pytest.raises(ValueError, match="batch_size must be >= 1"):
        local_logits(_model(), torch.zeros((6, 5)), batch_size=0)
    with pytest.raises(ValueError, match="no CPU fallback"):
        local_logits(_model(), torch.zeros((6, 5)))
    with pytest.raises(TypeError, match="no CPU fallback"):
        predict(None, torch.zeros((6, 5)), _model(), [0, 1], torch.zeros(6, dtype=torch.int64), "ppr", 2, infer=True)


def test_the_reddit_shaped_float64_chain_decides_every_row():
    """The seed and scales of infer_cases.reddit_pair, on the float64 reference alone: no row's top-2 gap is inside twice
    the rule's bound, and the predictions spread over the classes."""
    pred, decided = ic.reddit_chain64("ppr", 2, 0.2)
    assert bool(decided.all())
    counts = torch.bincount(pred, minlength=41)
    assert int((counts > 0).sum()) == 41 and int(counts.max()) < ic.N_NODES // 2
