"""CPU tests of the fused evaluation tail and the one-pass validation: the binding of csrc/eval_tail_abi.hpp in
_native.PRIVATE_ABI, the constants stated once, csrc/eval_plan.hpp itself (tests/native/eval_plan_check.cpp, built with the
address and undefined-behaviour sanitizers and run as a program) against the numpy mirror, the entry point's error codes
before any GPU work, every refusal of the Python layer before a device call, and the mirror's deliberate mistakes."""
import ctypes
import glob
import inspect
import os
import re

import numpy as np
import pytest
import torch

import abi_header as ah
import eval_tail_cases as tc
import native_check
from grand_plus_amd import _native
from grand_plus_amd import evaluate as ev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grand_plus_amd", "csrc")
P = ctypes.c_void_p(16)


# ---- 1. the binding and the constants
def test_the_table_is_the_headers_prototype_type_by_type():
    protos = ah.prototypes("eval_tail_abi.hpp")
    table = _native.PRIVATE_ABI["eval_tail_abi.hpp"]
    assert sorted(protos) == sorted(table) == ["gp_eval_tail"]
    (ret, params), (restype, argtypes, required) = protos["gp_eval_tail"], table["gp_eval_tail"]
    assert ah.expected_ctype("gp_eval_tail", *ret) is restype and not required
    assert [ah.expected_ctype("gp_eval_tail", base, stars, name) for base, stars, name in params] == argtypes
    # gp_eval_head's operands without the offset and the capacity, then gp_eval_reduce's from the workspace on, name by name
    pub = ah.prototypes("grandplus_eval.h")
    head = [p[2] for p in pub["gp_eval_head"][1]]
    red = [p[2] for p in pub["gp_eval_reduce"][1]]
    want = [n for n in head[:-1] if n not in ("out_offset", "out_capacity")] + red[red.index("d_workspace"):]
    assert [p[2] for p in params] == want


def test_the_unit_is_built_and_stays_outside_c_abi_4():
    import __graft_entry__ as entry
    assert "eval_tail.hip" in entry.LIB_UNITS
    for hdr in ("eval_tail_abi.hpp", "eval_head.hpp", "eval_plan.hpp"):
        assert os.path.join(CSRC, hdr) in entry.lib_sources()
    public = "".join(open(p).read() for p in glob.glob(os.path.join(ROOT, "include", "*.h")))
    assert "eval_tail" not in public and "EVAL_TAIL" not in public
    assert _native.lib().gp_abi_version() == 4
    tail, head = open(os.path.join(CSRC, "eval_tail.hip")).read(), open(os.path.join(CSRC, "evaluate.hip")).read()
    for unit in (tail, head):
        assert '#include "eval_head.hpp"' in unit and '#include "eval_plan.hpp"' in unit
        assert "GP_EVAL_HEAD_ROWS(a, nll, pred, flag)" in unit and "gp_eval::reduce_plan(n_rows)" in unit
    # the row arithmetic and the two lines of the plan are stated once
    for text, holder in (("bool better(", "eval_head.hpp"), ("#define GP_EVAL_HEAD_ROWS", "eval_head.hpp"), ("struct HeadArgs", "eval_head.hpp"),
                         ("ReducePlan reduce_plan(", "eval_plan.hpp"), ("/ kMinSlice", "eval_plan.hpp")):
        holders = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*")) if text in open(p, errors="replace").read())
        assert holders == [holder], (text, holders)
    code = re.sub(r"//[^\n]*", "", tail)
    # one returning ticket add and the reset; one release and one acquire; nothing that reads the host, spins or debugs
    assert re.findall(r"__hip_atomic_\w+", code) == ["__hip_atomic_fetch_add", "__hip_atomic_store"]
    assert re.findall(r"__ATOMIC_(?:RELEASE|ACQUIRE|ACQ_REL|SEQ_CST)", code) == ["__ATOMIC_RELEASE", "__ATOMIC_ACQUIRE"]
    assert code.index("__ATOMIC_RELEASE") < code.index("__hip_atomic_fetch_add") < code.index("__ATOMIC_ACQUIRE")
    assert not re.search(r"__threadfence|\bwhile\b|printf|\bassert\s*\(|hipMemcpy|hipMalloc|hipMemset|Synchronize", code)


def test_the_constants_are_stated_once_and_mirrored():
    text, code = ah.read("eval_tail_abi.hpp")
    assert int(re.search(r"#define GP_EVAL_TAIL_MAX_ROWS (\d+)", code).group(1)) == _native.EVAL_TAIL_MAX_ROWS == tc.TAIL_MAX_ROWS == 65536
    assert int(re.search(r"#define GP_EVAL_TAIL_WORKSPACE_BYTES (\d+)", code).group(1)) == _native.EVAL_TAIL_WORKSPACE_BYTES \
        == tc.TAIL_WORKSPACE_BYTES == 64
    plan = open(os.path.join(CSRC, "eval_plan.hpp")).read()
    assert re.findall(r"#include\s*[<\"]([^>\"]+)", plan) == ["cstdint"]
    assert tc.SLOTS * 40 == _native.eval_workspace_bytes()
    tail = open(os.path.join(CSRC, "eval_tail.hip")).read()
    assert "GP_EVAL_TAIL_MAX_ROWS == gp_eval::kTailMaxRows" in tail and "GP_EVAL_TAIL_WORKSPACE_BYTES == gp_eval::kTailWorkspaceBytes" in tail
    assert "kSlots == gp_eval::kSlots" in open(os.path.join(CSRC, "evaluate.hip")).read()
    sig = inspect.signature(ev.eval_tail).parameters
    assert list(sig)[:2] == ["logits", "labels"] and all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig)[2:])
    assert [sig[k].default for k in ("rows", "label_rows", "ignore_index", "out", "workspace")] == [None, None, -100, None, None]


# ---- 2. the plan header
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = native_check.build(tmp_path_factory, "eval_plan_check")

    def ask(lines):
        return native_check.ints(native_check.run(exe, lines))
    return ask


def test_the_plan_header_is_the_numpy_mirror(checker):
    assert checker(["consts"]) == [[tc.SLOTS, tc.MIN_SLICE, tc.TAIL_SLICES, tc.TAIL_MAX_ROWS, tc.TAIL_WORKSPACE_BYTES]]
    for n in tc.PLAN_N + (65537, 1024 * 1024, 1024 * 1024 + 1, 2 ** 40 + 3):
        (got,) = checker([f"plan {n}"])
        grid, rows = tc.plan(n)
        assert got[:2] == [grid, rows], n
        assert got[2:] == [0, min(rows, n), (grid - 1) * rows, min(n, grid * rows)], n
        assert grid * rows >= n and (grid - 1) * rows < max(n, 1)                   # the slices cover the rows, none is empty
        if n <= tc.TAIL_MAX_ROWS:
            assert grid <= tc.TAIL_SLICES and (n == 0 or rows <= tc.MIN_SLICE)
    assert [tc.plan(n) for n in tc.PLAN_N] == [(1, 0), (1, 1), (1, 1023), (1, 1024), (2, 513), (2, 1024), (3, 683), (64, 1024), (64, 1024)]
    assert tc.plan(65537)[0] == 65 > tc.TAIL_SLICES                                  # the first size past the cap needs one slice more


# ---- 3. error codes
def test_the_entry_returns_its_error_codes_before_any_gpu_work():
    """No device pointer here is real: every call has to stop at its argument checks."""
    E, N = _native.GP_ERR_INVALID_ARG, _native.GP_ERR_NULL
    L = _native.lib()

    def tail(z=P, R=10, C=7, rows=None, y=P, n_y=10, lrows=None, n=10, nll=P, pred=P, flag=P, ws=P, out=P, counts=P):
        return L.gp_eval_tail(0, z, R, C, rows, y, n_y, lrows, n, -100, nll, pred, flag, ws, out, counts, None)

    for kw in (dict(C=0), dict(C=4097), dict(n=-1), dict(R=-1), dict(n_y=-1), dict(n=65537, rows=P, lrows=P), dict(n=11), dict(n=11, rows=P),
               dict(n=11, lrows=P), dict(ws=ctypes.c_void_p(18))):
        assert tail(**kw) == E, kw
    assert "gp_eval_tail" in L.gp_last_error().decode()
    for name in ("z", "y", "nll", "pred", "flag", "ws", "out", "counts"):
        assert tail(**{name: None}) == N, name
    for name in ("ws", "out", "counts"):                                          # n_rows = 0 still writes the two NaNs
        assert tail(n=0, **{name: None}) == N, name
    assert tail(z=None, C=0) == E                                                 # sizes are judged first


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


def test_eval_tail_refuses_before_any_device_call(monkeypatch):
    _no_device(monkeypatch)
    z, y = torch.zeros(6, 7), torch.zeros(6, dtype=torch.int64)
    idx = torch.arange(4)
    with pytest.raises(TypeError, match="no CPU fallback"):
        ev.eval_tail(z, y)
    with pytest.raises(TypeError, match="no CPU fallback"):
        ev.eval_tail(z, y, rows=idx, label_rows=idx)
    for C in (0, 4097):
        with pytest.raises(ValueError, match=r"number of classes must be in \[1, 4096\]"):
            ev.eval_tail(torch.zeros(3, C), y)
    with pytest.raises(ValueError, match="rows has 4 entries, label_rows 3"):
        ev.eval_tail(z, y, rows=idx, label_rows=idx[:3])
    with pytest.raises(ValueError, match="label_rows has 7 entries, logits 6 rows"):
        ev.eval_tail(z, y, label_rows=torch.arange(7))
    with pytest.raises(ValueError, match="labels has 5 entries for 6 rows"):
        ev.eval_tail(z, y[:5])
    with pytest.raises(TypeError, match="float32"):
        ev.eval_tail(z.double(), y)
    with pytest.raises(TypeError, match="int64"):
        ev.eval_tail(z, y.int())
    with pytest.raises(TypeError, match="rows must be an int64"):
        ev.eval_tail(z, y, rows=idx.int())
    with pytest.raises(ValueError, match="do not fit the out buffers of 5"):
        ev.eval_tail(z, y, out=ev.eval_buffers(5, "cpu"))
    with pytest.raises(TypeError, match="workspace must be a contiguous uint8 tensor of at least 64 bytes"):
        ev.eval_tail(z, y, workspace=torch.zeros(63, dtype=torch.uint8))
    with pytest.raises(TypeError, match="result"):
        ev.eval_tail(z, y, result=(torch.zeros(2), torch.zeros(4)))


def _rows(n_seeds=3, K=4, n_nodes=12):
    from grand_plus_amd.rows import RowMatrix
    zz = torch.zeros(n_seeds * K, dtype=torch.int32)
    return RowMatrix(np.arange(n_seeds), K, zz, zz, torch.zeros(n_seeds * K, dtype=torch.float64), torch.full((n_seeds,), K, dtype=torch.int32),
                     n_nodes)


def test_one_pass_plans_refuse_before_any_device_call(monkeypatch):
    from grand_plus_amd import mag
    from grand_plus_amd.mlp import GrandPlusMLP, MagMLP
    _no_device(monkeypatch)
    assert inspect.signature(ev.valid_plan).parameters["one_pass"].default is False
    assert inspect.signature(ev.valid).parameters["one_pass"].default is False
    assert inspect.signature(ev.valid_pass).parameters["one_pass"].default is None
    assert inspect.signature(mag.valid_mag_plan).parameters["one_pass"].default is False
    assert inspect.signature(mag.valid_mag_pass).parameters["one_pass"].default is None
    assert ev.ValidPlan._fields == ("model", "rows", "features", "labels", "idx", "pos", "buf", "batch_size") and ev.ValidPlan.one is None
    assert mag.ValidMagPlan.one is None
    rows, X, y = _rows(), torch.zeros(12, 5), torch.zeros(12, dtype=torch.int64)
    m = GrandPlusMLP(5, 7, 8, 2, False, 0.0, 0.0, False)
    with pytest.raises(TypeError, match="no CPU fallback"):
        ev.valid_plan(m, rows, X, [0, 1], y, one_pass=True)
    for bad in (1, "yes", None):
        with pytest.raises(TypeError, match="one_pass and fused must be bools"):
            ev.valid_plan(m, rows, _fake(X), [0, 1], _fake(y), one_pass=bad)
    with pytest.raises(ValueError, match="fused=True needs one_pass=True"):
        ev.valid_plan(m, rows, _fake(X), [0, 1], _fake(y), fused=True)
    wide = GrandPlusMLP(5, 4097, 8, 2, False, 0.0, 0.0, False)
    with pytest.raises(ValueError, match=r"number of classes must be in \[1, 4096\], got 4097"):
        ev.valid_plan(wide, rows, _fake(X), [0, 1], _fake(y), one_pass=True)
    with pytest.raises(TypeError, match="one_pass=True needs a GrandPlusMLP or MagMLP"):
        ev.valid_plan(torch.nn.Linear(5, 7), rows, _fake(X), [0, 1], _fake(y), one_pass=True)
    mm = MagMLP(20, 4097, 8, 2, False, 0.0, 0.0, False)
    with pytest.raises(TypeError, match="no CPU fallback"):
        mag.valid_mag_plan(mm, rows, torch.zeros(13, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), torch.zeros(3), [0], y, one_pass=True)
    # a batched plan has no logits to run one pass over
    plan = ev.ValidPlan(m, rows, X, y, torch.zeros(0, dtype=torch.int64), None, ev.eval_buffers(0, "cpu"), 5)
    with pytest.raises(ValueError, match="needs a plan made with one_pass=True"):
        ev.valid_pass(plan, one_pass=True)
    with pytest.raises(TypeError, match="one_pass must be None"):
        ev.valid_pass(plan, one_pass=1)


def test_valid_graph_and_fit_refuse_before_any_device_call(monkeypatch):
    from grand_plus_amd import fit as fitm
    from grand_plus_amd.mlp import GrandPlusMLP
    _no_device(monkeypatch)
    m = GrandPlusMLP(5, 7, 8, 2, False, 0.0, 0.0, False)
    plan = ev.ValidPlan(m, _rows(), torch.zeros(12, 5), torch.zeros(12, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), None,
                        ev.eval_buffers(0, "cpu"), 5)
    assert list(inspect.signature(ev.ValidGraph.__init__).parameters) == ["self", "plan", "dropnode_rate", "tracker", "state"]

    class Tracker:
        buf = torch.zeros(5, dtype=torch.int64)

        def update(self, *a):
            pytest.fail("the tracker was reached")

    with pytest.raises(ValueError, match="a tracker needs the StepState"):
        ev.ValidGraph(plan, 0.5, Tracker())
    with pytest.raises(ValueError, match="a tracker needs the StepState"):
        ev.ValidGraph(plan, 0.5, Tracker(), state=object())
    with pytest.raises(TypeError, match="tracker must be a fit.BestTracker"):
        ev.ValidGraph(plan, 0.5, object(), state=object())
    with pytest.raises(TypeError, match="ValidGraph takes a ValidPlan"):
        ev.ValidGraph((m, 1, 2))
    with pytest.raises(ValueError, match=r"dropnode_rate must be in \[0, 1\]"):
        ev.ValidGraph(plan, 1.5)
    g = ev.ValidGraph(plan)
    assert g.runs == 0 and g.tracker is None
    for name in ("fit", "FitLoop"):
        sig = inspect.signature(getattr(fitm, name)).parameters
        assert sig["valid_one_pass"].default is False and sig["valid_capture"].default is False
        assert sig["valid_one_pass"].kind is inspect.Parameter.KEYWORD_ONLY
    from grand_plus_amd.mag_step import MagTrainStep
    from grand_plus_amd.step import TrainStep
    for cls in (TrainStep, MagTrainStep):
        assert inspect.signature(cls._valid_plan).parameters["one_pass"].default is False


# ---- 5. the mirror's deliberate mistakes
def test_the_cases_hold_flags_of_all_four_kinds():
    cases = tc.buffer_cases()
    kinds = set()
    for nll, flag in cases.values():
        kinds |= set(flag.tolist())
    assert kinds == {tc.WRONG, tc.CORRECT, tc.IGNORED, tc.BAD}
    assert set(cases[f"spread{tc.SPREAD_N}"][1].tolist()) == kinds
    lo, hi = tc.spread_nll(tc.SPREAD_N).min(), tc.spread_nll(tc.SPREAD_N).max()
    assert lo < 1e-5 and hi > 1e2                                                 # spread over 1e-6 ... 1e3


def test_the_gpu_inputs_hold_rows_of_all_four_kinds():
    """The label mix of tests/test_gpu_eval_tail.py, judged on the CPU: from 255 rows on and with more than one class every
    case has wrong, correct, ignored and bad rows, a NaN logit and a row of equal logits."""
    for n in (255, 256, 257, 1023, 1024, 1025, 2049, 4097):
        for C in (7, 64, 65):
            z, y = (t.numpy() for t in tc.mixed_case(n, C))
            pred = np.argmax(z, axis=1)
            flag = np.where(y == -100, tc.IGNORED, np.where((y < 0) | (y >= C), tc.BAD, np.where(pred == y, tc.CORRECT, tc.WRONG)))
            assert set(flag.tolist()) == {tc.WRONG, tc.CORRECT, tc.IGNORED, tc.BAD}, (n, C)
            assert np.isnan(z[1]).sum() == 1 and (z[2] == 0.5).all()
    rows, lrows = (t.numpy() for t in tc.index_lists(5, 8, 10))
    assert (rows < 0).any() and (rows >= 8).any() and (lrows < 0).any() and (lrows >= 10).any()


def test_the_mirror_is_the_plain_sum_where_order_cannot_matter():
    for name, (nll, flag) in tc.buffer_cases().items():
        loss, acc, counts, _sum = tc.reduce_mirror(nll, flag)
        n = len(nll)
        want = [int((flag <= tc.CORRECT).sum()), int((flag == tc.CORRECT).sum()), int((flag == tc.IGNORED).sum()), int((flag == tc.BAD).sum())]
        assert counts == want and sum(counts[0:1] + counts[2:]) == n, name
        if counts[0]:
            exact = float(np.sum(nll.astype(np.float64))) / counts[0]
            assert abs(float(loss) - exact) <= 2.0 ** -23 * abs(exact), name     # one float32 rounding of a float64 sum
            assert tc.bits(acc) == tc.bits(np.float32(counts[1] / n)), name
        else:
            assert np.isnan(loss), name
    empty = tc.reduce_mirror(*tc.buffer_cases()["empty"])
    assert np.isnan(empty[0]) and np.isnan(empty[1]) and empty[2] == [0, 0, 0, 0]


@pytest.mark.parametrize("mistake", tc.MISTAKES)
def test_every_mistake_changes_what_some_case_expects(mistake):
    """DESIGN §7q's method on the tail's reduce: a mistake that no case can tell from the right answer by its bits would mean
    the cases do not cover it."""
    found = [name for name, (nll, flag) in tc.buffer_cases().items()
             if not tc.same(tc.reduce_mirror(nll, flag), tc.reduce_mirror(nll, flag, mistake))]
    assert found, f"no case tells {mistake} from the right answer"
    if mistake == "slot_order":                                   # only more than two slices can tell; it shows in the float64 sum
        assert f"spread{tc.SPREAD_N}" in found and all(tc.plan(len(tc.buffer_cases()[name][0]))[0] > 2 for name in found), found
        nll, flag = tc.buffer_cases()[f"spread{tc.SPREAD_N}"]
        assert tc.same(tc.reduce_mirror(nll, flag), tc.reduce_mirror(nll, flag, mistake), sum64=False)   # ... and the quotient hides it
    if mistake == "float32_accumulation":
        assert "absorb" in found


def test_the_spread_inputs_give_the_spread_sums():
    """The GPU case is drawn from logits: its nll, as float64 -log softmax gives it, is the target to a few ulps, so the case
    keeps the spread that makes the slot order show."""
    z, y = tc.spread_logits(tc.SPREAD_N)
    want = tc.spread_nll(tc.SPREAD_N).astype(np.float64)
    nll = -torch.log_softmax(z.double(), 1).gather(1, y[:, None])[:, 0].numpy()
    assert np.all(np.abs(nll - want) <= 1e-5 * want + 1e-9)
    flag = np.zeros(tc.SPREAD_N, dtype=np.uint8)
    assert not tc.same(tc.reduce_mirror(nll.astype(np.float32), flag), tc.reduce_mirror(nll.astype(np.float32), flag, "slot_order"))
