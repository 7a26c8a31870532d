"""CPU tests of the evaluation path: eval_head / eval_reduce / valid / predict refuse what they cannot run
before any launch (there is no CPU fallback), and the C entry points return their error codes before any GPU work."""
import ctypes
import re

import pytest
import torch

from grand_plus_amd import _native

P = ctypes.c_void_p(16)


def _z(n=6, C=3, dtype=torch.float32):
    return torch.zeros((n, C), dtype=dtype)


def _y(n=6, dtype=torch.int64):
    return torch.zeros(n, dtype=dtype)


def _buf(n):
    from grand_plus_amd.evaluate import eval_buffers
    return eval_buffers(n, "cpu")


def test_valid_and_predict_are_importable_from_the_package():
    import grand_plus_amd
    from grand_plus_amd import eval_head, eval_reduce, predict, valid
    for f in (eval_head, eval_reduce, predict, valid):
        assert f.__module__ == "grand_plus_amd.evaluate"
    assert not {"valid", "predict", "eval_head", "eval_reduce"} & set(grand_plus_amd.__all__)


# every tensor here is on the CPU: dtype, shape and size are refused before the device is looked at, each with its own message
@pytest.mark.parametrize("kw,exc,msg", [
    (dict(logits=_z(dtype=torch.float64)), TypeError, "logits must be a float32 [R, C]"),
    (dict(logits=_z(dtype=torch.float16)), TypeError, "logits must be a float32 [R, C]"),
    (dict(logits=torch.zeros(6)), TypeError, "logits must be a float32 [R, C]"),
    (dict(logits=_z(C=0)), ValueError, "classes must be in [1, 4096], got 0"),
    (dict(logits=_z(n=1, C=4097)), ValueError, "classes must be in [1, 4096], got 4097"),
    (dict(labels=_y(dtype=torch.int32)), TypeError, "labels must be an int64"),
    (dict(labels=None), TypeError, "labels must be an int64"),
    (dict(rows=_y(dtype=torch.int32)), TypeError, "rows must be an int64"),
    (dict(label_rows=_y(dtype=torch.float32)), TypeError, "label_rows must be an int64"),
    (dict(rows=_y(4), label_rows=_y(5)), ValueError, "rows has 4 entries, label_rows 5"),
    (dict(label_rows=_y(7)), ValueError, "label_rows has 7 entries, logits 6 rows"),
    (dict(labels=_y(5)), ValueError, "labels has 5 entries for 6 rows"),
    (dict(offset=-1), ValueError, "offset must be >= 0"),
    (dict(out=_buf(5)), ValueError, "offset + n = 6 rows do not fit the out buffers of 5"),
    (dict(out=_buf(8), offset=3), ValueError, "offset + n = 9 rows do not fit the out buffers of 8"),
    (dict(out=(torch.zeros(6), torch.zeros(6), torch.zeros(6))), TypeError, "out.pred must be a contiguous 1-d torch.int32"),
    (dict(out=_buf(6)[:2]), TypeError, "out must be the (nll, pred, flag) buffers"),
    (dict(), TypeError, "no CPU fallback"),
    (dict(out=_buf(6)), TypeError, "no CPU fallback"),
])
def test_eval_head_refuses_before_any_launch(kw, exc, msg, monkeypatch):
    from grand_plus_amd.evaluate import eval_head
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the native library was reached"))
    args = dict(logits=_z(), labels=_y())
    args.update(kw)
    with pytest.raises(exc, match=re.escape(msg)):
        eval_head(args.pop("logits"), args.pop("labels"), **args)


def test_eval_reduce_refuses_before_any_launch(monkeypatch):
    from grand_plus_amd.evaluate import eval_reduce
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the native library was reached"))
    with pytest.raises(TypeError, match="no CPU fallback"):
        eval_reduce(_buf(4))
    with pytest.raises(TypeError, match="out.flag"):
        eval_reduce((torch.zeros(4), torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)))
    with pytest.raises(ValueError, match="same length"):
        eval_reduce((torch.zeros(4), torch.zeros(4, dtype=torch.int32), torch.zeros(3, dtype=torch.uint8)))


def test_valid_and_predict_refuse_before_any_launch(monkeypatch):
    from grand_plus_amd import predict, valid
    from grand_plus_amd.mlp import GrandPlusMLP
    from grand_plus_amd.rows import RowMatrix
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the native library was reached"))
    model = GrandPlusMLP(5, 3, 4, 2, False, 0.0, 0.0, False).train()
    rm = RowMatrix([0, 1], 2, None, torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.float64),
                   torch.zeros(2, dtype=torch.int32), 6)
    X, y = torch.zeros((6, 5)), _y()
    with pytest.raises(TypeError, match="rows must be a RowMatrix"):
        valid(model, object(), X, [0, 1], y)
    with pytest.raises(TypeError, match="model must be"):
        valid(lambda x: x, rm, X, [0, 1], y)
    with pytest.raises(TypeError, match="features must be a contiguous float32"):
        valid(model, rm, X.double(), [0, 1], y)
    with pytest.raises(TypeError, match="labels must be an int64"):
        valid(model, rm, X, [0, 1], y.int())
    with pytest.raises(TypeError, match="no CPU fallback"):
        valid(model, rm, X, [0, 1], y)
    with pytest.raises(TypeError, match="features must be a contiguous float32"):
        predict(None, X.t(), model, [0, 1], y, "ppr", 2)
    with pytest.raises(TypeError, match="no CPU fallback"):
        predict(None, X, model, [0, 1], y, "ppr", 2)
    assert model.training                                            # nothing touched the model


def _head(logits=P, n_z=4, C=3, labels=P, n_labels=4, n=4, off=0, cap=4, nll=P, pred=P, flag=P, rows=None, lrows=None):
    return _native.lib().gp_eval_head(0, logits, n_z, C, rows, labels, n_labels, lrows, n, -100, off, cap, nll, pred, flag, None)


def test_entries_return_their_error_codes_before_any_gpu_work():
    """No device pointer here is real: every call has to stop at its argument checks."""
    E, N = _native.GP_ERR_INVALID_ARG, _native.GP_ERR_NULL
    assert _head(C=0) == E and _head(C=4097) == E
    assert "gp_eval_head" in _native.lib().gp_last_error().decode()
    assert _native.GP_MAX_CLASSES == 4096 and _head(C=-1) == E and _head(C=2 ** 31 - 1) == E
    assert _head(C=4096, n=0, cap=0, nll=None) == _native.GP_OK      # the limit itself passes the checks
    assert _head(n=-1) == E and _head(n_z=-1) == E and _head(n_labels=-1) == E and _head(off=-1) == E
    assert _head(off=1) == E and _head(cap=3) == E and _head(off=2 ** 62, cap=2 ** 62) == E     # past the buffers
    assert _head(n_z=3) == E and _head(n_labels=3) == E                # more rows than the array, no index list
    assert _head(n_z=3, rows=P, nll=None) == N                         # ... with one the sizes pass
    assert _head(logits=None) == N and _head(labels=None) == N and _head(pred=None) == N and _head(flag=None) == N
    assert _head(n=0, cap=0, nll=None) == _native.GP_OK                # nothing to do, nothing touched
    red = _native.lib().gp_eval_reduce
    assert red(0, P, P, -1, P, P, P, None) == E
    assert "gp_eval_reduce" in _native.lib().gp_last_error().decode()
    assert red(0, None, P, 1, P, P, P, None) == N and red(0, P, None, 1, P, P, P, None) == N
    assert red(0, None, None, 0, None, P, P, None) == N and red(0, None, None, 0, P, None, P, None) == N
    assert red(0, None, None, 0, P, P, None, None) == N
