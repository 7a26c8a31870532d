"""CPU tests of the fused inference path: the C entry point returns its error codes before any GPU work,
`infer(fused=True)` and `predict(fused=True)` refuse what they cannot run before any launch, and fused=False reaches
none of the new code."""
import ctypes
import re

import pytest
import torch

import infer_chain_cases as cc
from grand_plus_amd import _native

P = ctypes.c_void_p(16)


def _call(x=P, n=4, f_in=3, f_hidden=5, f_out=2, w1=P, b1=P, flags1=0, g1=P, be1=P, rm1=P, rv1=P, eps1=1e-5,
          w2=P, b2=P, flags2=0, g2=P, be2=P, rm2=P, rv2=P, eps2=1e-5, out=P, ws=P):
    return _native.lib().gp_mlp_infer_chain2(0, x, n, f_in, f_hidden, f_out, w1, b1, flags1, g1, be1, rm1, rv1, eps1,
                                             w2, b2, flags2, g2, be2, rm2, rv2, eps2, out, ws, None)


def test_the_entry_returns_its_error_codes_before_any_gpu_work():
    """No device pointer here is real: every call has to stop at its argument checks."""
    E, N, OK = _native.GP_ERR_INVALID_ARG, _native.GP_ERR_NULL, _native.GP_OK
    R, NORM, BN, TR = _native.GP_MLP_RELU, _native.GP_MLP_NORM, _native.GP_MLP_BN, _native.GP_MLP_TRAINING
    assert _call(n=-1) == E
    assert "gp_mlp_infer_chain2" in _native.lib().gp_last_error().decode()
    assert _call(f_in=0) == E and _call(f_hidden=0) == E and _call(f_out=0) == E and _call(f_in=-3) == E
    assert _call(f_hidden=1025) == E
    assert "gp_mlp_infer_chain2" in _native.lib().gp_last_error().decode() and "1024" in _native.lib().gp_last_error().decode()
    assert _call(f_out=65) == E and _call(f_hidden=2 ** 22) == E and _call(f_hidden=1025, f_out=65) == E
    for key in ("flags1", "flags2"):
        assert _call(**{key: TR}) == E and _call(**{key: R | NORM | BN | TR}) == E
        assert _call(**{key: 16}) == E and _call(**{key: -1}) == E
    assert _call(n=2 ** 40 + 1) == E and _call(f_in=2 ** 31 - 1, f_hidden=1024) == E
    assert _call(f_in=2 ** 31 - 1, f_hidden=1) == E and _call(f_in=2 ** 31 - 31, f_hidden=1) == E      # k + 31 has to stay an int
    assert _call(flags1=BN, eps1=0.0) == E and _call(flags1=BN, eps1=-1.0) == E and _call(flags1=BN, eps1=float("nan")) == E
    assert _call(flags2=BN, eps2=0.0) == E and _call(flags2=BN, eps2=-1.0) == E and _call(flags2=BN, eps2=float("nan")) == E
    assert _call(x=None) == N and _call(w1=None) == N and _call(w2=None) == N and _call(out=None) == N
    assert _call(flags1=BN, rm1=None) == N and _call(flags1=BN, rv1=None) == N
    assert _call(flags2=BN, rm2=None) == N and _call(flags2=BN, rv2=None) == N
    for key in ("flags1", "flags2"):
        assert _call(ws=None, **{key: NORM}) == N and _call(ws=None, **{key: BN}) == N and _call(ws=None, **{key: R | NORM | BN}) == N
    # nothing to do: GP_OK, nothing launched, the pointers not looked at
    assert _call(n=0) == OK
    assert _call(n=0, x=None, w1=None, w2=None, out=None, ws=None, flags1=R | NORM | BN, flags2=R | NORM | BN) == OK
    assert _call(n=0, flags2=TR) == E and _call(n=0, f_hidden=1025) == E and _call(n=0, f_out=65) == E


def _grand(F=5, C=3, H=4, nl=2):
    from grand_plus_amd.mlp import GrandPlusMLP
    return GrandPlusMLP(F, C, H, nl, True, 0.5, 0.5, True).train()


def _mag(C=3, H=4, nl=2):
    from grand_plus_amd.mlp import MagMLP
    return MagMLP(9, C, H, nl, True, 0.5, 0.5, True).train()


# every tensor here is on the CPU: the limits of the fused kernel are refused before the device is looked at
@pytest.mark.parametrize("make,width,msg", [
    (lambda: _grand(nl=1), 5, "fewer than two blocks"),
    (lambda: _mag(nl=2), 4, "fewer than two blocks"),          # the MAG layout's first layer is the embedding
    (lambda: _mag(nl=1), 3, "fewer than two blocks"),
    (lambda: _grand(H=1025), 5, "hidden size 1025 is above the limit of 1024"),
    (lambda: _grand(H=1025, nl=3), 5, "hidden size 1025 is above the limit of 1024"),
    (lambda: _mag(H=1025, nl=3), 1025, "hidden size 1025 is above the limit of 1024"),
    (lambda: _grand(C=65), 5, "65 classes are above the limit of 64"),
    (lambda: _grand(H=1024, C=64), 5, "no CPU fallback"),      # at the limits: only the device is missing
    (lambda: _grand(nl=3), 5, "no CPU fallback"),
])
def test_fused_infer_refuses_before_any_launch(make, width, msg, monkeypatch):
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the native library was reached"))
    model = make()
    with pytest.raises(ValueError, match=re.escape(msg)):
        model.infer(torch.zeros((6, width)), fused=True)
    assert model.training


def test_local_logits_and_predict_refuse_before_any_launch(monkeypatch):
    from grand_plus_amd import local_logits, predict
    from grand_plus_amd.mag import predict_mag
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the native library was reached"))
    with pytest.raises(ValueError, match="fewer than two blocks"):
        local_logits(_grand(nl=1), torch.zeros((6, 5)), fused=True)
    with pytest.raises(ValueError, match="above the limit of 64"):
        local_logits(_grand(C=65), torch.zeros((6, 5)), fused=True)
    y = torch.zeros(6, dtype=torch.int64)
    with pytest.raises(ValueError, match="fused=True needs infer=True"):
        predict(None, torch.zeros((6, 5)), _grand(), [0, 1], y, "ppr", 2, fused=True)
    with pytest.raises(ValueError, match="fused=True needs infer=True"):
        predict(None, torch.zeros((6, 5)), _grand(), [0, 1], y, "ppr", 2, infer=False, fused=True)
    import inspect
    for fn in (predict, predict_mag, local_logits):
        assert inspect.signature(fn).parameters["fused"].default is False
    assert inspect.signature(predict).parameters["infer"].default is False


def test_unfused_infer_reaches_none_of_the_new_code(monkeypatch):
    """fused=False is the path of before: with the chain's binding, its workspace mirror and its limits all raising, the
    host checks of `infer` still run to their last one."""
    from grand_plus_amd import mlp

    def boom(*_a, **_k):
        raise AssertionError("fused=False reached the fused path")

    monkeypatch.setattr(mlp, "_infer_chain2", boom)
    monkeypatch.setattr(_native, "mlp_infer_chain_workspace_bytes", boom)
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the native library was reached"))
    for model in (_grand(nl=1), _grand(H=1025), _grand(C=65), _grand()):      # shapes the fused path refuses, too
        with pytest.raises(ValueError, match="no CPU fallback"):
            model.infer(torch.zeros((6, 5)))
        with pytest.raises(ValueError, match="no CPU fallback"):
            model.infer(torch.zeros((6, 5)), fused=False)
    with pytest.raises(ValueError, match="no CPU fallback"):
        mlp._check_infer(torch.zeros((6, 5)), None, None, _grand(C=65)._layers())


def test_the_shared_cases_are_the_multi_block_ones_and_the_others_are_refused(monkeypatch):
    """The case table of the GPU test: every multi-block case of infer_cases is in it, and the one-block ones (pubmed,
    aminer, and mag: the MAG layout's first layer is the embedding) are what `infer(fused=True)` refuses."""
    import infer_cases as ic
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the native library was reached"))
    names = [c[0] for c in cc.CASES]
    assert len(names) == len(set(names))
    assert {"cora", "citeseer", "reddit", "amazon2m", "deep", "mag_bn", "deep33_bn_norm", "deep33_plain", "f48"} == set(names)
    assert [c[0] for c in cc.ONE_BLOCK] == ["pubmed", "aminer", "mag"]
    assert cc.ROWS == (1, 31, 32, 33, 63, 64, 65, 129, 300) and cc.B == 70
    for case in cc.ONE_BLOCK:
        m = cc.model(case)
        assert len(m._layers()) == 1
        with pytest.raises(ValueError, match="fewer than two blocks"):
            m.infer(ic.inputs(case, 3), fused=True)
    for case in cc.CASES + [cc.MAG_LARGE, cc.CHUNK]:           # these pass the fused limits: only the device is missing
        m = cc.model(case)
        assert len(m._layers()) >= 2
        with pytest.raises(ValueError, match="no CPU fallback"):
            m.infer(ic.inputs(case, 3), fused=True)
