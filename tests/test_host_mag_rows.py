"""CPU tests of MAG's fused front end: the C entry points return their error codes before any GPU work,
`mag_prop_rows` / `valid_mag` / `predict_mag` refuse what they cannot run before any launch (there is no CPU fallback),
`mag_slot_seed` is the header's formula, the order contract's own float32 rounding stays inside the tolerance of every
case, and the valid_mag inputs are decided in float64."""
import ctypes
import os
import re

import pytest
import torch

import abi_header
import evaluate_cases as ec
import mag_cases as mc
from grand_plus_amd import _common, _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(16)
NAMES = ["gp_mag_prop_rows", "gp_mag_prop_rows_backward"]


def test_the_public_names_are_importable_from_the_package():
    import grand_plus_amd
    from grand_plus_amd import mag_prop_rows, predict_mag, valid_mag
    for f in (mag_prop_rows, valid_mag, predict_mag):
        assert f.__module__ == "grand_plus_amd.mag" and f.__name__ not in grand_plus_amd.__all__
    from grand_plus_amd.mlp import MagMLP
    assert callable(MagMLP.emb_rows)


def _call(name, w=P, V=5, H=4, ip=P, ix=P, dt=P, N=3, col=P, val=P, filled=P, S_rows=2, K=3, rows=P, B=2, S=1, p_node=0.5, p_in=0.0,
          training=1, keep=None, stride=6, out=P, n_bad=P):
    tail = (out, n_bad, None) if name == NAMES[0] else (out, None)
    return getattr(_native.lib(), name)(0, w, V, H, ip, ix, dt, N, col, val, filled, S_rows, K, rows, B, S, p_node, p_in, training,
                                        ctypes.c_uint64(7), keep, stride, *tail)


@pytest.mark.parametrize("name", NAMES)
def test_the_entries_return_their_error_codes_before_any_gpu_work(name):
    """No device pointer here is real: every call has to stop at its argument checks."""
    E, N, OK = _native.GP_ERR_INVALID_ARG, _native.GP_ERR_NULL, _native.GP_OK
    call = lambda **kw: _call(name, **kw)                                          # noqa: E731
    assert call(S=_native.GP_MAX_SAMPLES + 1) == E
    assert name in _native.lib().gp_last_error().decode()
    assert call(S=0) == E and call(S=-1) == E
    assert call(K=0) == E and call(K=_native.GP_MAX_K + 1) == E and call(K=-4) == E
    assert call(H=0) == E and call(H=-1) == E and call(V=0) == E
    for p in (-0.1, 1.5, float("nan")):
        assert call(p_node=p) == E and call(p_in=p) == E
    assert call(B=-1) == E and call(S_rows=-1) == E and call(N=-1) == E
    assert call(keep=P, stride=0) == E
    for missing in ("w", "ip", "ix", "dt", "col", "val", "out"):
        assert call(**{missing: None}) == N, missing
    # nothing to do: GP_OK, nothing launched, the pointers not looked at; but the arguments are still checked
    assert call(B=0) == OK and call(B=0, w=None, out=None, col=None) == OK
    assert call(B=0, K=0) == E and call(B=0, S=17) == E and call(B=0, p_in=2.0) == E


@pytest.mark.parametrize("seed,s,e", [(0, 0, 0), (1, 0, 0), (0x5EED0FACADE, 3, 191), (2 ** 64 - 1, 15, 2 ** 31 + 5), (123456789, 1, 1023)])
def test_mag_slot_seed_is_the_formula_of_the_header(seed, s, e):
    text, _ = abi_header.read("grandplus_mag.h")
    m = re.search(r"GP_MAG_SLOT_SEED\(seed, s, e\) = mix\(gp_sample_seed\(seed, s\) \^ \(\(e \+ 1\) \* (0x[0-9A-F]{16})\)\)", text)
    assert m, "the header states the formula"
    mul = int(m.group(1), 16)
    assert mul % 2 == 1
    hip = open(os.path.join(ROOT, "grand_plus_amd", "csrc", "mag_prop.hip")).read()
    shared = open(os.path.join(ROOT, "grand_plus_amd", "csrc", "gp_common.hpp")).read()
    assert m.group(1) + "ull" in hip and m.group(1) not in shared                    # no other derivation uses the constant
    M = 2 ** 64 - 1
    want = _common._mix(_common.sample_seed(seed, s) ^ (((e + 1) * mul) & M))
    assert _common.mag_slot_seed(seed, s, e) == want and 0 <= want <= M
    assert _common.mag_slot_seed(seed, s, e) != _common.mag_slot_seed(seed, s, e + 1)
    assert _common.mag_slot_seed(seed, s, e) != _common.layer_seed(seed, e, s)


def test_fixed_vectors_of_the_slot_seed_and_the_hash():
    """Values worked out once from the formulas (splitmix64's finaliser): a change of either formula shows here."""
    M = 2 ** 64 - 1

    def fmix(x):
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
        return x ^ (x >> 31)

    seed, e = 42, 5
    want = fmix(((seed ^ ((e + 1) * 0xE7037ED1A0B428DB & M)) + 0x9E3779B97F4A7C15) & M)
    assert _common.mag_slot_seed(seed, 0, e) == want
    keep = mc.hash_keep(want, range(8), 0.5)
    u = [((fmix((want + t * 0x9E3779B97F4A7C15) & M)) >> 40) / 16777216.0 for t in range(8)]
    assert keep.tolist() == [x >= 0.5 for x in u]


# every tensor here is on the CPU: type, shape and size are refused before the device is looked at
def _host_args(**kw):
    c = mc.case("h7_k5_s3")
    Pm = c["P"]
    a = dict(weight=Pm.W, attr_indptr=Pm.indptr, attr_indices=Pm.indices, attr_data=Pm.data, col=Pm.col.reshape(-1),
             val=Pm.val.reshape(-1), filled=Pm.filled, K=Pm.K)
    a.update(kw)
    return a


@pytest.mark.parametrize("kw,exc,msg", [
    (dict(samples=0), ValueError, "samples must be an int"),
    (dict(samples=17), ValueError, "samples must be an int"),
    (dict(samples=2.0), ValueError, "samples must be an int"),
    (dict(deterministic="yes"), TypeError, "deterministic must be None, True or False"),
    (dict(weight=None), TypeError, "weight must be a contiguous CUDA tensor"),
    (dict(), TypeError, "weight must be a contiguous CUDA tensor"),
])
def test_mag_prop_rows_refuses_before_any_launch(kw, exc, msg, monkeypatch):
    from grand_plus_amd import mag_prop_rows
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the native library was reached"))
    a = _host_args(**kw)
    with pytest.raises(exc, match=re.escape(msg)):
        mag_prop_rows(a.pop("weight"), a.pop("attr_indptr"), a.pop("attr_indices"), a.pop("attr_data"), a.pop("col"), a.pop("val"),
                      a.pop("filled"), a.pop("K"), **a)


def test_valid_mag_and_predict_mag_refuse_before_any_launch(monkeypatch):
    from grand_plus_amd import predict_mag, valid_mag
    from grand_plus_amd.mlp import GrandPlusMLP, MagMLP
    from grand_plus_amd.rows import RowMatrix
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the native library was reached"))
    ip, ix, dt = mc.mag_attributes(10)
    y = torch.zeros(10, dtype=torch.int64)
    mag = MagMLP(mc.MAG_V, 3, 8, 2, True, 0.0, 0.5, True).train()
    rm = RowMatrix([0, 1], 2, None, torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.float64), torch.zeros(2, dtype=torch.int32), 10)
    with pytest.raises(TypeError, match="model must be a MagMLP"):
        valid_mag(GrandPlusMLP(5, 3, 4, 2, True, 0.5, 0.5, True), rm, ip, ix, dt, [0], y)
    with pytest.raises(TypeError, match="rows must be a RowMatrix"):
        valid_mag(mag, None, ip, ix, dt, [0], y)
    with pytest.raises(TypeError, match="labels must be an int64"):
        valid_mag(mag, rm, ip, ix, dt, [0], y.int())
    with pytest.raises(ValueError, match="batch_size must be >= 1"):
        valid_mag(mag, rm, ip, ix, dt, [0], y, batch_size=0)
    with pytest.raises(TypeError, match="no CPU fallback"):
        valid_mag(mag, rm, ip, ix, dt, [0], y)
    with pytest.raises(TypeError, match="rows must be a RowMatrix"):
        mag.emb_rows(ip, ix, dt, (rm.col, rm.val))
    with pytest.raises(TypeError, match="model must be a MagMLP"):
        predict_mag(None, ip, ix, dt, GrandPlusMLP(5, 3, 4, 2, True, 0.5, 0.5, True), [0], y, "ppr", 2)
    with pytest.raises(TypeError, match="CUDA tensor"):
        predict_mag(None, ip, ix, dt, mag, [0], y, "ppr", 2)
    assert mag.training and torch.is_grad_enabled()


def test_the_order_contract_in_float32_stays_inside_the_tolerance_of_every_case():
    worst = 0.0
    for name in mc.CASES:
        c = mc.case(name)
        kw = c["kw"]
        got = mc.emulate(c["P"], c["batch"], c["S"], kw["dropnode_rate"], kw["input_droprate"], kw["training"], c["keep"], mc.SEED)
        ratio = mc.close(got, c["ref"][0], c["ref"][1], c["roundings"], name)
        print(f"[mag] {name}: {c['roundings']} roundings, emulated error / bound {ratio:.3g}")
        worst = max(worst, ratio)
    print(f"[mag] worst emulated error / bound {worst:.3g}")
    assert worst <= 1.0


def test_the_cases_cover_the_shapes_the_kernel_branches_on():
    H, K, S, bags = (set(c[i] for c in mc.CASES.values()) for i in (0, 1, 2, 8))
    assert {1, 7, 64, 65, 130} <= H and {1, 5, 32} <= K and {1, 2, 3, 16} <= S
    assert set(mc.BAGS) == {0, 1, 63, 64, 65, 130} and mc.BAGS in bags
    assert {c[3] for c in mc.CASES.values()} == {"ragged", "full", None} and {c[4] for c in mc.CASES.values()} == {None, "reversed", "repeat"}
    c = mc.case("h64_k32_s2")["P"]
    assert int(c.filled[0]) == 0 and int(c.filled[1]) == 32 and bool((c.col[:, 0] == 3).all()) and int(c.col[1, 31]) == 3
    assert mc.case("hub")["P"].longest == 4097 and mc.case("hub")["roundings"] > mc.ROUNDINGS


def test_the_valid_mag_inputs_are_decided_in_float64():
    """The cap on undecided rows is met by the reference alone, and the predictions are not all one class."""
    w, _ours, r64 = mc.valid_reference()
    left_out = 1.0 - float(r64["decided"].double().mean())
    counts = torch.bincount(r64["pred"], minlength=mc.MAG_C)
    print(f"[mag] valid_mag reference: {left_out:.4f} of the rows within the margin, predictions per class {counts.tolist()}")
    assert left_out <= ec.LEFT_OUT
    assert int((counts > 0).sum()) >= 4 and int(counts.max()) < 0.6 * w["idx_val"].numel()
