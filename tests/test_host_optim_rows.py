"""CPU tests of the embedding table's row-list step: csrc/optim_rows_layout.hpp itself
(tests/native/optim_rows_check.cpp, built with the address and undefined-behaviour sanitizers and run as a program) against
brute force, what is particular to the entry points of csrc/optim_rows_abi.hpp in _native.PRIVATE_ABI (tests/test_host_abi.py
holds the types), their error codes before any GPU work, every refusal of the Python layer before a device call, and the
numpy mirror's deliberate mistakes."""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import abi_header as ah
import native_check
import optim_rows_cases as rc
from grand_plus_amd import _native
from grand_plus_amd import optim_rows as orows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grand_plus_amd", "csrc")
P = ctypes.c_void_p(16)
NAMES = ["gp_clip_adam_rows", "gp_clip_adam_rows_dev", "gp_optim_rows_sqnorm"]
VS = (1, 5, 64, 4097)


# ---- 1. the layout header
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = native_check.build(tmp_path_factory, "optim_rows_check")

    def ask(V, keys):
        out = native_check.ints(native_check.run(exe, [f"list {V} " + " ".join(map(str, keys))]))
        assert len(out) == 4
        return out
    return ask


def test_the_layout_header_needs_nothing_but_the_standard_library(tmp_path):
    layout = open(os.path.join(CSRC, "optim_rows_layout.hpp")).read()
    assert re.findall(r"#include\s*[<\"]([^>\"]+)", layout) == ["cstdint"]
    src = tmp_path / "only_layout.cpp"
    src.write_text('#include "optim_rows_layout.hpp"\nint main() { long long k[2] = {0, 3}; return (int)gp_optim_rows::lower_bound(k, 2, 9) - 2; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-o", str(tmp_path / "only_layout"), str(src)], check=True,
                   timeout=120)
    subprocess.run([str(tmp_path / "only_layout")], check=True, timeout=60)


@pytest.mark.parametrize("V", VS)
def test_heads_and_lower_bounds_are_brute_force(checker, V):
    """Every key list of the grid -- the lengths 0, 1, 63, 64, 65 and 1 025, runs of 1, 63, 64 and 65 equal keys, a run that
    starts at position 63, keys below 0 and at or above V, the all-sentinel list, rows 0 and V - 1 -- from the header under
    the sanitizers."""
    lists = rc.key_lists(V)
    assert {len(lists[f"n{n}"]) for n in rc.N_SORTED} == set(rc.N_SORTED)
    for name, keys in lists.items():
        got_heads, got_lb, got_touched, (got_windows,) = checker(V, keys)
        assert got_heads == rc.heads(keys, V), name
        assert got_lb == [rc.lower_bound(keys, row) for row in range(-1, V + 2)], name
        assert got_touched == rc.touched(keys, V).astype(int).tolist(), name
        assert got_windows == (len(keys) + 63) // 64
        # a touched row has exactly one head, and the lower bound finds it
        assert sorted(int(keys[i]) for i in got_heads) == np.flatnonzero(rc.touched(keys, V)).tolist(), name
        for i in got_heads:
            assert got_lb[int(keys[i]) + 1] == i


def test_the_grid_holds_the_edges_it_names():
    for V in VS:
        lists = rc.key_lists(V)
        assert lists["run_at_63"][62] != lists["run_at_63"][63] == lists["run_at_63"][132] == V - 1
        assert rc.heads(lists["run_at_63"], V) == [63] and rc.heads(lists["all_sentinel"], V) == [] and rc.heads(lists["n0"], V) == []
        assert lists["out_of_range"][0] < 0 and lists["out_of_range"][-1] > V
        assert {0, V - 1} <= set(lists["edges"].tolist()) and rc.heads(lists["tail_window"], V) == [64]
    runs = rc.key_lists(64)["runs"]
    assert sorted(np.unique(runs[runs < 64], return_counts=True)[1].tolist()) == sorted(rc.RUNS)
    assert len(rc.stride_keys()) == rc.STRIDE_N and (rc.STRIDE_N + 63) // 64 > 2 * rc.GRID_CAP * rc.WAVES


# ---- 2. the binding
def test_the_table_is_the_headers_prototypes_type_by_type():
    """The generic part -- every type by the convention, the library's exports -- is tests/test_host_abi.py's."""
    protos, code = ah.prototypes("optim_rows_abi.hpp"), ah.read("optim_rows_abi.hpp")[1]
    assert sorted(protos) == sorted(_native.PRIVATE_ABI["optim_rows_abi.hpp"]) == NAMES
    # the pair mirrors the dense pair: the same arguments but for the two corrections, by value or by device pointer
    a, b = protos["gp_clip_adam_rows"][1], protos["gp_clip_adam_rows_dev"][1]
    assert len(a) == len(b) == 21 and [x for x, y in zip(a, b) if x != y] == [("float", 0, "step_size"), ("float", 0, "rsqrt_bc2")]
    assert [y for x, y in zip(a, b) if x != y] == [("float", 1, "d_step_size"), ("float", 1, "d_rsqrt_bc2")]
    dense = ah.prototypes("grandplus.h")["gp_clip_adam_step"][1]
    assert [p[2] for p in a[10:]] == [p[2] for p in dense[4:]]                    # max_norm .. stream, name by name
    modes = dict(re.findall(r"#define (GP_OPTIM_ROWS_[A-Z]+) (\d+)", code))
    assert {k: int(v) for k, v in modes.items()} == {"GP_OPTIM_ROWS_EXACT": orows.MODES["exact"], "GP_OPTIM_ROWS_LAZY": orows.MODES["lazy"]}


def test_the_entry_points_stay_outside_c_abi_4():
    import __graft_entry__ as entry
    assert "optim_rows.hip" in entry.LIB_UNITS
    for hdr in ("optim_rows_abi.hpp", "optim_rows_layout.hpp", "optim_math.hpp"):
        assert os.path.join(CSRC, hdr) in entry.lib_sources()
    public = "".join(open(p).read() for p in glob.glob(os.path.join(ROOT, "include", "*.h")))
    assert "optim_rows" not in public and "adam_rows" not in public and "GP_OPTIM_ROWS" not in public
    mag_det_abi = open(os.path.join(CSRC, "mag_det_abi.hpp")).read()
    assert "optim_rows" not in mag_det_abi and "adam_rows" not in mag_det_abi
    assert not [n for n in vars(_native) if "OPTIM_ROWS" in n.upper()]
    assert _native.lib().gp_abi_version() == 4


def test_the_arithmetic_is_stated_once_and_the_unit_holds_no_atomics():
    hip = open(os.path.join(CSRC, "optim_rows.hip")).read()
    dense = open(os.path.join(CSRC, "optim.hip")).read()
    for hdr in ("optim_math.hpp", "optim_rows_layout.hpp", "optim_rows_abi.hpp"):
        assert f'#include "{hdr}"' in hip
    assert '#include "optim_math.hpp"' in dense
    for name in ("struct AdamArgs", "void adam_element(", "float clip_coef("):
        holders = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*")) if name in open(p, errors="replace").read())
        assert holders == ["optim_math.hpp"], (name, holders)
    for text in (hip, dense):
        code = re.sub(r"//[^\n]*", "", text)
        assert "adam_element(" in code and "clip_coef<kWaves>(" in code
        assert not re.search(r"1e-6f|sqrtf|\(float\)sqrt", code), "the norm or the element update written out again"
    code = re.sub(r"//[^\n]*", "", hip)
    assert not re.search(r"atomic|\basm\b|printf|\bassert\s*\(|__builtin_amdgcn_s_|hipMemcpy|hipMalloc|Synchronize", code)
    for call in ("gp_optim_rows::is_head(", "gp_optim_rows::touched(", "gp_optim_rows::windows("):
        assert call in code, call
    assert "lower_bound(keys, n_sorted, row)" in open(os.path.join(CSRC, "optim_rows_layout.hpp")).read().split("bool touched")[1]
    # the lines tests/second_trip_cases.py reads stay in optim.hip
    for line in ("constexpr int kChunk = 4096;", "constexpr int kSlots = GP_OPTIM_WORKSPACE_BYTES / 8;", "constexpr int kMaxGrid = kSlots;"):
        assert dense.count(line) == 1, line
    assert rc.CHUNK == int(re.search(r"constexpr int kRowsChunk = (\d+);", hip).group(1))
    assert rc.GRID_CAP == _native.optim_workspace_bytes() // 8 and rc.WAVES == 256 // 64


# ---- 3. error codes
def test_the_entries_return_their_error_codes_before_any_gpu_work():
    """No device pointer here is real: every call has to stop at its argument checks."""
    E, N, OK = _native.GP_ERR_INVALID_ARG, _native.GP_ERR_NULL, _native.GP_OK
    L = _native.lib()

    def sq(keys=P, n=10, V=50, H=7, dW=P, acc=0, ws=P):
        return L.gp_optim_rows_sqnorm(0, keys, n, V, H, dW, acc, ws, None)

    for kw in (dict(n=-1), dict(V=0), dict(V=-3), dict(H=0), dict(H=-1), dict(V=2 ** 62, H=4)):
        assert sq(**kw) == E, kw
    assert "gp_optim_rows_sqnorm" in L.gp_last_error().decode()
    for name in ("keys", "dW", "ws"):
        assert sq(**{name: None}) == N, name
    assert sq(keys=None, V=0) == E                                                # sizes are judged first
    assert sq(n=0, acc=1) == OK                                                   # nothing to add: nothing launched

    def adam(entry="gp_clip_adam_rows", p=P, m=P, v=P, dW=P, keys=P, n=10, V=50, H=7, mode=1, max_norm=0.1, lr=1e-2, b1=0.9, b2=0.999,
             eps=1e-8, wd=0.0, step=P, rsq=P, ws=P, norm=P):
        corr = (0.1, 1.0) if entry == "gp_clip_adam_rows" else (step, rsq)
        return getattr(L, entry)(0, p, m, v, dW, keys, n, V, H, mode, max_norm, lr, b1, b2, eps, wd, *corr, ws, norm, None)

    for entry in ("gp_clip_adam_rows", "gp_clip_adam_rows_dev"):
        for kw in (dict(mode=0), dict(mode=3), dict(mode=-1), dict(n=-1), dict(V=0), dict(H=0), dict(max_norm=float("nan")),
                   dict(lr=float("inf")), dict(b1=float("nan")), dict(eps=float("inf")), dict(wd=float("nan")),
                   dict(mode=2, wd=5e-4), dict(mode=2, wd=-1e-3), dict(mode=2, wd=5e-4, n=0)):
            assert adam(entry, **kw) == E, (entry, kw)
        assert entry in L.gp_last_error().decode()
        assert adam(entry, mode=2, wd=1e-3) == E and "lazy" in L.gp_last_error().decode()
        for name in ("p", "m", "v", "dW", "keys", "ws", "norm"):
            assert adam(entry, **{name: None}) == N, (entry, name)
        assert adam(entry, p=None, mode=7) == E
        assert adam(entry, mode=2, n=0) == OK                                     # lazy, nothing touched: nothing launched
    for name in ("step", "rsq"):
        assert adam("gp_clip_adam_rows_dev", **{name: None}) == N, name


# ---- 4. the Python layer
class _Cuda(torch.Tensor):
    """A CPU tensor that says it is on the GPU: it passes the type checks of the Python layer, which must refuse before it
    reaches the library."""
    @property
    def is_cuda(self):
        return True


def _fake(t):
    return t.as_subclass(_Cuda)


def _no_device(monkeypatch):
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the native library was reached"))


def test_row_grad_refuses_what_is_no_table(monkeypatch):
    _no_device(monkeypatch)
    for bad in (None, [1.0], torch.zeros(3, 4, dtype=torch.float64), torch.zeros(4, 6)[:, ::2]):
        with pytest.raises(TypeError, match="dense contiguous float32"):
            orows.RowGrad(bad)
    for bad in (torch.zeros(4), torch.zeros(2, 3, 4), torch.zeros(0, 4), torch.zeros(4, 0)):
        with pytest.raises(ValueError, match=r"2-D \[V, H\]"):
            orows.RowGrad(bad)
    with pytest.raises(TypeError, match="no CPU fallback"):
        orows.RowGrad(torch.zeros(4, 3))
    w = _fake(torch.zeros(4, 3))
    rg = orows.RowGrad(w)
    assert rg.values.shape == (4, 3) and rg.values.dtype == torch.float32 and rg.keys is None and rg.n_sorted == 0 and not rg.filled()
    for bad in ("dense", "Exact", None, 1):
        with pytest.raises(ValueError, match="'exact' or 'lazy'"):
            orows.check_mode(bad)
    import grand_plus_amd
    assert grand_plus_amd.RowGrad is orows.RowGrad and "RowGrad" not in grand_plus_amd.__all__


def test_mag_prop_rows_refuses_a_row_grad_before_any_device_call(monkeypatch):
    import mag_cases as mc
    from grand_plus_amd.mag import mag_prop_rows
    from grand_plus_amd.mlp import MagMLP
    _no_device(monkeypatch)
    Pm = mc.case("h7_k5_s3")["P"]
    a = dict(attr_indptr=Pm.indptr, attr_indices=Pm.indices, attr_data=Pm.data, col=Pm.col.reshape(-1), val=Pm.val.reshape(-1),
             filled=Pm.filled)
    a = {k: _fake(v) for k, v in a.items()}
    w = _fake(Pm.W.clone().requires_grad_(True))
    rg = orows.RowGrad(w)
    with pytest.raises(TypeError, match="row_grad must be an optim_rows.RowGrad"):
        mag_prop_rows(w, **a, K=Pm.K, deterministic=True, max_entries=100, row_grad=torch.zeros(3))
    for kw in (dict(deterministic=False, max_entries=100), dict(max_entries=100), dict(deterministic=True)):     # the atomic mode
        with pytest.raises(ValueError, match="row_grad needs the deterministic backward"):
            mag_prop_rows(w, **a, K=Pm.K, row_grad=rg, **kw)
    other = _fake(Pm.W.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="made for another tensor"):
        mag_prop_rows(other, **a, K=Pm.K, deterministic=True, max_entries=100, row_grad=rg)
    rg.shape = (Pm.W.shape[0] + 1, Pm.W.shape[1])                                 # the wrong shape
    with pytest.raises(ValueError, match="row_grad holds a"):
        mag_prop_rows(w, **a, K=Pm.K, deterministic=True, max_entries=100, row_grad=rg)
    rg.shape, rg.device = tuple(Pm.W.shape), torch.device("meta")                 # the wrong device
    with pytest.raises(ValueError, match="row_grad holds a"):
        mag_prop_rows(w, **a, K=Pm.K, deterministic=True, max_entries=100, row_grad=rg)
    import inspect
    assert inspect.signature(mag_prop_rows).parameters["row_grad"].default is None
    assert inspect.signature(MagMLP.emb_rows).parameters["row_grad"].default is None


def test_clip_adam_refuses_a_row_grad_before_any_device_call(monkeypatch):
    from grand_plus_amd import ClipAdam
    _no_device(monkeypatch)
    w, b = torch.nn.Parameter(_fake(torch.zeros(4, 3))), torch.nn.Parameter(_fake(torch.zeros(3)))
    rg = orows.RowGrad(w)
    opt = ClipAdam([w, b], weight_decay=5e-4)
    with pytest.raises(TypeError, match="row_grad must be an optim_rows.RowGrad"):
        opt.set_row_grad(w, object(), "exact")
    with pytest.raises(ValueError, match="'exact' or 'lazy'"):
        opt.set_row_grad(w, rg, "sparse")
    with pytest.raises(ValueError, match="not a parameter of this optimiser"):
        opt.set_row_grad(torch.nn.Parameter(torch.zeros(4, 3)), rg, "exact")
    with pytest.raises(ValueError, match="made for another tensor"):
        opt.set_row_grad(b, rg, "exact")
    with pytest.raises(ValueError, match="'lazy' takes weight_decay = 0"):
        opt.set_row_grad(w, rg, "lazy")
    assert not opt._row_grads
    opt.set_row_grad(w, rg, "exact")
    b.grad = _fake(torch.zeros(3))
    with pytest.raises(RuntimeError, match="no backward has filled"):             # a step before any backward
        opt.step()
    assert not opt.state
    rg.fill(torch.zeros(2, dtype=torch.int64))
    w.grad = _fake(torch.zeros(4, 3))
    with pytest.raises(ValueError, match="also has a dense .grad"):
        opt.step()
    w.grad = None
    lazy = ClipAdam([w], weight_decay=0.0)
    lazy.set_row_grad(w, rg, "lazy")
    lazy.param_groups[0]["weight_decay"] = 1e-3                                   # changed after set_row_grad: step() looks again
    with pytest.raises(ValueError, match="'lazy' takes weight_decay = 0"):
        lazy.step()
    assert not lazy.state and not opt.state


class _FakeState:
    device = torch.device("cuda", 0)

    def configure(self, *a):
        pass


def test_mag_train_step_refuses_a_table_step_before_any_device_call(monkeypatch):
    import inspect

    from test_host_mag_det import _mag_step
    from grand_plus_amd import ClipAdam, MagTrainStep, mag_trained_parameters
    from grand_plus_amd.mlp import MagMLP
    _no_device(monkeypatch)
    assert inspect.signature(MagTrainStep.__init__).parameters["table_step"].default is None
    for bad in ("dense", "Lazy", 1, True):
        with pytest.raises(ValueError, match="'exact' or 'lazy'"):
            _mag_step(table_step=bad, deterministic=True)
    for mode in ("exact", "lazy"):
        with pytest.raises(ValueError, match="needs the deterministic table gradient"):
            _mag_step(table_step=mode, deterministic=False)
        with pytest.raises(ValueError, match="needs the deterministic table gradient"):
            _mag_step(table_step=mode)                                            # torch's flag is off
        with pytest.raises(ValueError, match="no CPU fallback"):                  # everything else passes: only the device is missing
            _mag_step(table_step=mode, deterministic=True)
    # a capturable optimiser accepts a parameter whose gradient is a RowGrad, and still refuses one with neither
    model = MagMLP(9, 3, 4, 2, True, 0.0, 0.5, True).train()
    opt = ClipAdam(mag_trained_parameters(model), capturable=True, state=_FakeState())
    for p in mag_trained_parameters(model)[1:]:
        p.grad = torch.zeros_like(p)
    with pytest.raises(ValueError, match="a parameter has no gradient"):
        opt._check_capturable()
    opt._row_grads[model.embeds.weight] = (object(), "exact")
    opt._check_capturable()


# ---- 5. the mirror's deliberate mistakes
HYPER = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, clip=0.1)


def _mirror(mode, V, H, keys, mistake=None):
    p, m, v = rc.state(V, H, 3)
    dW = rc.gradient(keys, V, H, 5)
    step_size, rsqrt_bc2 = rc.corrections(HYPER["lr"], HYPER["betas"], 3)
    return rc.mirror_step(mode, p, m, v, dW, keys, step_size=step_size, rsqrt_bc2=rsqrt_bc2, mistake=mistake, **HYPER)


def _differs(a, b):
    return any(not rc.same_bits(x, y) for x, y in zip(a[:3], b[:3])) or not rc.same_bits(np.float32(a[3]), np.float32(b[3]))


@pytest.mark.parametrize("mistake", rc.MISTAKES)
def test_every_mistake_changes_what_some_case_expects(mistake):
    """DESIGN §7q's method on the row list: a mistake that no case of the grid can tell from the right answer would mean the
    grid does not cover it.  The unmistaken mirror, for its part, never lets a NaN of dW's poison into the table."""
    V, H = 5, 7
    found = []
    for name, keys in rc.key_lists(V).items():
        for mode in rc.MODES:
            right = _mirror(mode, V, H, keys)
            assert all(np.isfinite(x).all() for x in right[:3]) and np.isfinite(right[3]), (name, mode)
            if _differs(right, _mirror(mode, V, H, keys, mistake)):
                found.append((name, mode))
    assert found, f"no case of the grid tells {mistake} from the right step"
    want_mode = {"lazy_decays_untouched": "lazy", "exact_skips_untouched": "exact", "exact_reads_untouched_dW": "exact"}.get(mistake)
    if want_mode:
        assert {mode for _, mode in found} == {want_mode}
    want_case = {"pos0_not_head": "run_from_0", "oob_key_as_row": "out_of_range", "run_crossing_64_twice": "run_at_63",
                 "last_window_dropped": "tail_window"}.get(mistake)
    if want_case:
        assert want_case in {name for name, _ in found}, found


def test_the_mirror_in_both_modes():
    V, H = 5, 7
    keys = rc.key_lists(V)["runs"]
    t = rc.touched(keys, V)
    assert t.any() and not t.all()
    p0, m0, v0 = rc.state(V, H, 3)
    pe, me, ve, ne = _mirror("exact", V, H, keys)
    pl, ml, vl, nl = _mirror("lazy", V, H, keys)
    assert ne == nl and ne > 0
    for e, l, old in ((pe, pl, p0), (me, ml, m0), (ve, vl, v0)):
        assert rc.same_bits(e[t], l[t]) and rc.same_bits(l[~t], old[~t])           # lazy: touched rows as exact, the rest untouched
        assert not rc.same_bits(e[~t], old[~t])                                    # exact: an untouched row still moves (dense Adam)
    # exact mode is the dense step on the zero-filled gradient
    dense = rc.dense_gradient(rc.gradient(keys, V, H, 5), keys)
    all_rows = np.arange(V, dtype=np.int64)
    step_size, rsqrt_bc2 = rc.corrections(HYPER["lr"], HYPER["betas"], 3)
    pd, md, vd, nd = rc.mirror_step("exact", p0, m0, v0, dense, all_rows, step_size=step_size, rsqrt_bc2=rsqrt_bc2, **HYPER)
    assert rc.same_bits(pd, pe) and rc.same_bits(md, me) and rc.same_bits(vd, ve) and nd == ne
