"""CPU tests of the embedding table's deferred exact Adam step: csrc/optim_defer_layout.hpp itself
(tests/native/optim_defer_check.cpp, built with the address and undefined-behaviour sanitizers and run as a program) against the
numpy mirror of the bookkeeping, what is particular to the entry points of csrc/optim_defer_abi.hpp in _native.PRIVATE_ABI
(tests/test_host_abi.py holds the types), their error codes before any GPU work, every refusal of the Python layer before a
device call, and the mirror's deliberate mistakes."""
import ctypes
import glob
import inspect
import os
import re

import pytest
import torch

import abi_header as ah
import native_check
import optim_defer_cases as dc
from grand_plus_amd import _native
from grand_plus_amd import optim_rows as orows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grand_plus_amd", "csrc")
P = ctypes.c_void_p(16)
NAMES = ["gp_optim_defer_catch_up", "gp_optim_defer_flush", "gp_optim_defer_step"]
SCENARIOS = {"main": dc.main, "wrap": dc.wrap, "single_row": dc.single_row, "largest_gap": lambda: dc.past_the_gap(0),
             "past_the_gap": lambda: dc.past_the_gap(1)}
JUMP = (4, 6)                 # before step 4 the tick moves to 6 without a reset: steps 4 and 5 never stood in the ring


# ---- 1. the layout header
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = native_check.build(tmp_path_factory, "optim_defer_check")
    return lambda lines: native_check.ints(native_check.run(exe, lines))


def _program(sc, pre_forward=True, jump=None):
    """The scenario as queries of the check program, and the final tick."""
    lines, T = [f"new {sc.V} {sc.capacity} 0"], 0
    for t in range(1, sc.n_steps + 1):
        T = jump[1] if jump and jump[0] == t else T + 1
        rows = " ".join(map(str, sc.touches[t]))
        if pre_forward:
            lines.append(f"catch {T} {rows}")
        lines.append(f"step {T} {rows}")
        if t in sc.flush_after:
            lines.append(f"flush {T}")
    return lines + ["dump"], T


def test_the_layout_header_needs_nothing_but_the_standard_library():
    layout = open(os.path.join(CSRC, "optim_defer_layout.hpp")).read()
    assert re.findall(r"#include\s*[<\"]([^>\"]+)", layout) == ["cstdint"]
    code = re.sub(r"//[^\n]*", "", layout)
    assert "sizeof(Entry) == 16" in code and "kFlagBit = %d;" % dc.FLAG_BIT in code
    assert "kMinCapacity = %d;" % dc.MIN_CAPACITY in code and "kMaxCapacity = %d;" % dc.MAX_CAPACITY in code
    assert (orows.DEFER_MIN_CAPACITY, orows.DEFER_MAX_CAPACITY, orows.DEFER_FLAG_BIT) == (dc.MIN_CAPACITY, dc.MAX_CAPACITY, dc.FLAG_BIT)


@pytest.mark.parametrize("name", sorted(SCENARIOS))
@pytest.mark.parametrize("pre_forward", [True, False], ids=["catch-up", "inline"])
def test_the_header_keeps_the_books_as_the_mirror_does(checker, name, pre_forward):
    """Every scenario through the header under the sanitizers, with and without the pre-forward call: last and the flag."""
    sc = SCENARIOS[name]()
    lines, _ = _program(sc, pre_forward)
    last, (flag,) = checker(lines)
    book, T = dc.run_book(sc, pre_forward=pre_forward)
    assert last == book.last.tolist() and flag == book.flag
    if name == "past_the_gap":
        assert flag == dc.FLAG_BIT and last[1] == 1 and all(x == T for i, x in enumerate(last) if i != 1)
        assert book.applied[1] == [1] and all(a == list(range(1, T + 1)) for i, a in enumerate(book.applied) if i != 1)
    else:                                                              # flushed at the end: every row on the dense trajectory
        assert flag == 0 and last == [T] * sc.V
        assert all(a == list(range(1, T + 1)) for a in book.applied)


def test_a_tick_that_jumps_or_a_stale_slot_is_flagged_not_replayed(checker):
    sc = dc.main()
    lines, T = _program(sc, jump=JUMP)
    last, (flag,) = checker(lines)
    book, T2 = dc.run_book(sc, jump=JUMP)
    assert T == T2 == sc.n_steps + 2 and flag == book.flag == dc.FLAG_BIT and last == book.last.tolist()
    assert max(last) == JUMP[0] - 1                                    # every row lagged across the jump: all stay where they were
    # one slot's tag overwritten: the rows whose replay reads it keep their last, the others are served
    lines = [f"new 6 {dc.CAPACITY} 0"] + [f"step {t} 0" for t in range(1, 8)] + ["tamper 5 99", "catch 8 1", "step 8 0 1", "flush 8", "dump"]
    last, (flag,) = checker(lines)
    assert last == [8, 0, 0, 0, 0, 0] and flag == dc.FLAG_BIT


def test_plan_on_both_sides_of_every_edge(checker):
    C = dc.CAPACITY
    queries = {(20, 19, 19, C): 0, (20, 20, 19, C): 0, (20, 18, 19, C): 1, (20, 20 - C, 19, C): 1, (20, 20 - C, 20, C): 1,
               (20, 19 - C, 19, C): 2, (20, 19 - C, 20, C): 2, (20, 21, 20, C): 2, (20, -1, 19, C): 2, (0, 0, -1, C): 0,
               (2 ** 31 - 1, 2 ** 31 - 2, 2 ** 31 - 1, C): 1, (2 ** 31, 2 ** 31 - 1, 2 ** 31, C): 2,
               (70000, 70000 - 65536, 70000, 65536): 1, (70000, 70000 - 65537, 70000, 65536): 2}
    got = checker([("plan %d %d %d %d" % q) for q in queries])
    assert [g[0] for g in got] == list(queries.values())
    for (tick, last, through, cap), want in queries.items():
        assert {"nothing": 0, "replay": 1, "unserved": 2}[dc.Book(1, cap)._plan(tick, last, through)] == want
    caps = [-8, 0, 1, 2, 3, 4, 5, 8, 12, 1024, 65536, 65537, 131072]
    assert [g[0] for g in checker([f"cap {c}" for c in caps])] == [int(4 <= c <= 65536 and c & (c - 1) == 0) for c in caps]
    for c in caps:
        if 4 <= c <= 65536 and c & (c - 1) == 0:
            assert orows.check_capacity(c) == c
        else:
            with pytest.raises(ValueError, match="power of two"):
                orows.check_capacity(c)
    assert orows.check_capacity(None) == orows.DEFER_CAPACITY == 1024
    for bad in (8.0, "8", True):
        with pytest.raises(ValueError, match="power of two"):
            orows.check_capacity(bad)


def test_the_scenarios_hold_the_edges_they_name():
    C = dc.CAPACITY
    assert {1, 2, C - 1, C} <= dc.gaps_seen(dc.main()) and max(dc.gaps_seen(dc.main())) == C
    main = dc.main()
    assert len(main.touches[5]) == 0 and all(len(main.touches[t]) for t in range(1, 25) if t != 5)
    assert all(0 in main.touches[t] for t in range(1, 25) if t != 5) and not any(1 in a for a in main.touches.values())
    assert main.V - 1 in main.touches[7] and main.V % 64 and main.n_steps > 2 * C
    wrap = dc.wrap()
    assert wrap.n_steps > 2 * C and max(dc.gaps_seen(wrap)) == C
    assert max(dc.gaps_seen(dc.past_the_gap(0))) == C and max(dc.gaps_seen(dc.past_the_gap(1))) == C + 1
    for kind in dc.KINDS:
        keys = dc.key_list([3, 7, 96], dc.V, kind)
        assert (keys[1:] >= keys[:-1]).all() and keys[-1] == dc.V and sorted({int(keys[i]) for i in dc.rc.heads(keys, dc.V)}) == [3, 7, 96]
    assert len(dc.key_list([3, 7, 96], dc.V, "det", 1)) > len(dc.key_list([3, 7, 96], dc.V, "bitmap"))
    assert len(dc.key_list([], dc.V, "bitmap")) == 3 and not dc.rc.heads(dc.key_list([], dc.V, "det"), dc.V)
    # the kernels' constants as the cases state them
    hip = open(os.path.join(CSRC, "optim_defer.hip")).read()
    for name, value in (("kCatchGrid", dc.CATCH_GRID), ("kFlushGrid", dc.FLUSH_GRID), ("kBlock", dc.WAVES * 64)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, hip).group(1)) == value, name
    assert "constexpr int kStepGrid = kSlots;" in hip and dc.STEP_GRID == _native.optim_workspace_bytes() // 8
    assert {h % 64 for h in dc.HS} >= {0, 3, 4} and dc.V == 97


# ---- 2. the binding
def test_the_table_is_the_headers_prototypes_type_by_type():
    """The generic part -- every type by the convention, the library's exports -- is tests/test_host_abi.py's."""
    protos = ah.prototypes("optim_defer_abi.hpp")
    assert sorted(protos) == sorted(_native.PRIVATE_ABI["optim_defer_abi.hpp"]) == NAMES
    for name, (ret, params) in protos.items():
        restype, argtypes, required = _native.PRIVATE_ABI["optim_defer_abi.hpp"][name]
        assert required is False and restype is ah.expected_ctype(name, *ret)
        assert argtypes == [ah.expected_ctype(name, *p) for p in params], name
        # the deferred state travels the same way in all three, right before what ends the call
        names = [p[2] for p in params]
        at = names.index("d_tick")
        assert names[at:at + 5] == ["d_tick", "d_last", "d_hist", "capacity", "d_flag"] and names[-1] == "stream"
    # the step is gp_clip_adam_rows_dev without a mode, with the deferred state before the workspace
    rows = [p[2] for p in ah.prototypes("optim_rows_abi.hpp")["gp_clip_adam_rows_dev"][1]]
    step = [p[2] for p in protos["gp_optim_defer_step"][1]]
    assert [n for n in step if n not in ("d_tick", "d_last", "d_hist", "capacity", "d_flag")] == [n for n in rows if n != "mode"]
    built = ctypes.CDLL(_native.LIB_PATH)
    assert all(hasattr(built, name) for name in NAMES)


def test_the_unit_is_built_and_states_nothing_twice():
    import __graft_entry__ as entry
    assert "optim_defer.hip" in entry.LIB_UNITS
    for hdr in ("optim_defer_abi.hpp", "optim_defer_layout.hpp", "optim_rows_heads.hpp"):
        assert os.path.join(CSRC, hdr) in entry.lib_sources()
    public = "".join(open(p).read() for p in glob.glob(os.path.join(ROOT, "include", "*.h")))
    assert "optim_defer" not in public
    hip = open(os.path.join(CSRC, "optim_defer.hip")).read()
    code = re.sub(r"//[^\n]*", "", hip)
    for hdr in ("optim_math.hpp", "optim_rows_layout.hpp", "optim_rows_heads.hpp", "optim_defer_layout.hpp", "optim_defer_abi.hpp"):
        assert f'#include "{hdr}"' in hip
    # the arithmetic is optim_math.hpp's, called with the literal zero in the replay; nothing of it is typed again
    assert code.count("adam_element(p, 0.0f, m, v, lane_value(e.coef, j), b);") == 1 and "clip_coef<kWaves>(" in code
    assert not re.search(r"1e-6f|sqrtf|\(float\)sqrt|weight_decay \*|beta1 \*|beta2 \*", code)
    assert not re.search(r"atomic|\basm\b|printf|\bassert\s*\(|hipMemcpy|hipMalloc|Synchronize", code)
    for call in ("gp_optim_defer::plan(", "gp_optim_defer::tag_ok(", "gp_optim_defer::slot(", "gp_optim_defer::tag(",
                 "gp_optim_defer::valid_capacity(", "gp_optim_rows::is_head(", "gp_optim_rows::windows(", "take_heads("):
        assert call in code, call
    # take_heads is stated once, in the header both row-list units include
    holders = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*")) if "int take_heads(" in open(p, errors="replace").read())
    assert holders == ["optim_rows_heads.hpp"]
    assert '#include "optim_rows_heads.hpp"' in open(os.path.join(CSRC, "optim_rows.hip")).read()


# ---- 3. error codes
def test_the_entries_return_their_error_codes_before_any_gpu_work():
    """No device pointer here is real: every call has to stop at its argument checks."""
    E, N, OK = _native.GP_ERR_INVALID_ARG, _native.GP_ERR_NULL, _native.GP_OK
    L = _native.lib()
    base = dict(p=P, m=P, v=P, dW=P, keys=P, n=10, V=50, H=7, max_norm=0.1, lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=1e-3, step=P, rsq=P,
                tick=P, last=P, hist=P, cap=8, flag=P, ws=P, norm=P)

    def catch(**kw):
        a = dict(base, **kw)
        return L.gp_optim_defer_catch_up(0, a["p"], a["m"], a["v"], a["keys"], a["n"], a["V"], a["H"], a["b1"], a["b2"], a["eps"], a["wd"],
                                         a["tick"], a["last"], a["hist"], a["cap"], a["flag"], None)

    def step(**kw):
        a = dict(base, **kw)
        return L.gp_optim_defer_step(0, a["p"], a["m"], a["v"], a["dW"], a["keys"], a["n"], a["V"], a["H"], a["max_norm"], a["lr"], a["b1"],
                                     a["b2"], a["eps"], a["wd"], a["step"], a["rsq"], a["tick"], a["last"], a["hist"], a["cap"], a["flag"],
                                     a["ws"], a["norm"], None)

    def flush(**kw):
        a = dict(base, **kw)
        return L.gp_optim_defer_flush(0, a["p"], a["m"], a["v"], a["V"], a["H"], a["b1"], a["b2"], a["eps"], a["wd"], a["tick"], a["last"],
                                      a["hist"], a["cap"], a["flag"], None)

    common = [dict(V=0), dict(V=-3), dict(H=0), dict(H=-1), dict(V=2 ** 62, H=4), dict(b1=float("nan")), dict(b2=float("inf")),
              dict(eps=float("inf")), dict(wd=float("nan"))] + [dict(cap=c) for c in (0, 2, 3, 12, 1000, 65537, 131072, -8)]
    pointers = ["p", "m", "v", "tick", "last", "hist", "flag"]
    for name, f, more_bad, more_ptr in (("gp_optim_defer_catch_up", catch, [dict(n=-1)], ["keys"]),
                                        ("gp_optim_defer_step", step, [dict(n=-1), dict(max_norm=float("nan")), dict(lr=float("inf"))],
                                         ["keys", "dW", "step", "rsq", "ws", "norm"]),
                                        ("gp_optim_defer_flush", flush, [], [])):
        for kw in common + more_bad:
            assert f(**kw) == E, (name, kw)
        assert name in L.gp_last_error().decode()
        for ptr in pointers + more_ptr:
            assert f(**{ptr: None}) == N, (name, ptr)
        assert f(p=None, cap=5) == E                                               # sizes are judged first
    assert catch(cap=5) == E and "power of two" in L.gp_last_error().decode()
    assert catch(n=0) == OK                                                        # nothing is listed: nothing launched
    for cap in (4, 65536):
        assert catch(n=0, cap=cap) == OK
    # weight decay is allowed, with either sign
    assert catch(n=0, wd=5e-4) == OK and catch(n=0, wd=-1e-3) == OK


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


def test_the_mode_exists_beside_the_two_it_leaves_alone():
    assert orows.MODES["deferred"] not in (orows.MODES["exact"], orows.MODES["lazy"]) and sorted(orows.MODES) == ["deferred", "exact", "lazy"]
    assert orows.check_mode("deferred") == "deferred"
    for bad in ("dense", "Deferred", None, 3):
        with pytest.raises(ValueError, match="'deferred'"):
            orows.check_mode(bad)
    assert "DeferredRows" in orows.__all__


def test_clip_adam_refuses_a_deferred_table_before_any_device_call(monkeypatch):
    from grand_plus_amd import ClipAdam
    _no_device(monkeypatch)
    w, b = torch.nn.Parameter(_fake(torch.zeros(4, 3))), torch.nn.Parameter(_fake(torch.zeros(3)))
    rg = orows.RowGrad(w)
    opt = ClipAdam([w, b], weight_decay=5e-4)
    with pytest.raises(ValueError, match="needs ClipAdam\\(capturable=True"):
        opt.set_row_grad(w, rg, "deferred")
    with pytest.raises(ValueError, match="needs ClipAdam\\(capturable=True"):
        opt.set_row_grad(w, rg, "deferred", capacity=8)
    for mode in ("exact", "lazy"):
        with pytest.raises(ValueError, match="belong to mode 'deferred'"):
            opt.set_row_grad(w, rg, mode, capacity=8)
    assert not opt._row_grads and not opt._deferred
    opt.flush_rows()                                                               # no deferred table: nothing to do, nothing reached
    assert list(inspect.signature(ClipAdam.set_row_grad).parameters) == ["self", "param", "row_grad", "mode", "capacity", "flag"]
    assert inspect.signature(ClipAdam.set_row_grad).parameters["capacity"].default is None

    class _State:
        device = torch.device("cpu")
        buf = torch.zeros(11, dtype=torch.int64)

        def configure(self, *a):
            pass

    cap = ClipAdam([w, b], weight_decay=5e-4, capturable=True, state=_State())
    for bad in (0, 3, 12, 131072, 8.0):
        with pytest.raises(ValueError, match="power of two"):
            cap.set_row_grad(w, rg, "deferred", capacity=bad)
    with pytest.raises(ValueError, match="not a parameter of this optimiser"):
        cap.set_row_grad(torch.nn.Parameter(torch.zeros(4, 3)), rg, "deferred")
    with pytest.raises(ValueError, match="made for another tensor"):
        cap.set_row_grad(b, rg, "deferred")
    with pytest.raises(TypeError, match="flag must be an int32 tensor of one element"):
        cap.set_row_grad(w, rg, "deferred", flag=torch.zeros(2, dtype=torch.int32))
    assert not cap._row_grads and not cap._deferred
    # weight decay is allowed; the state is device memory of the object, made without the library
    cap.set_row_grad(w, rg, "deferred", capacity=8)
    d = cap.deferred_rows(w)
    assert isinstance(d, orows.DeferredRows) and d.capacity == 8 and d.last.shape == (4,) and d.last.dtype == torch.int32
    assert d.hist.numel() * 4 == 8 * 16 and d.flag.dtype == torch.int32 and d.flag.numel() == 1
    cap.set_row_grad(w, rg, "exact")                                               # back to another mode: the deferred state goes
    assert not cap._deferred


def test_mag_train_step_refuses_a_deferred_table_before_any_device_call(monkeypatch):
    from test_host_mag_det import _mag_step
    from grand_plus_amd import MagTrainStep
    _no_device(monkeypatch)
    sig = inspect.signature(MagTrainStep.__init__).parameters
    assert sig["defer_capacity"].default is None and sig["table_step"].default is None
    assert callable(MagTrainStep.flush_table)
    with pytest.raises(ValueError, match="needs the deterministic table gradient"):
        _mag_step(table_step="deferred", deterministic=False)
    with pytest.raises(ValueError, match="needs the deterministic table gradient"):
        _mag_step(table_step="deferred")                                           # torch's flag is off
    with pytest.raises(ValueError, match="it needs deterministic=False"):
        _mag_step(table_step="deferred", row_list="bitmap", deterministic=True)
    for kw in (dict(deterministic=True), dict(deterministic=False, row_list="bitmap")):
        with pytest.raises(ValueError, match="dirty_rows=True needs table_step='lazy'"):
            _mag_step(table_step="deferred", dirty_rows=True, **kw)
        for bad in (0, 3, 12, 131072, "8"):
            with pytest.raises(ValueError, match="power of two"):
                _mag_step(table_step="deferred", defer_capacity=bad, **kw)
        with pytest.raises(ValueError, match="no CPU fallback"):                   # everything else passes: only the device is missing
            _mag_step(table_step="deferred", defer_capacity=8, **kw)
    for mode in (None, "exact", "lazy"):
        with pytest.raises(ValueError, match="defer_capacity belongs to table_step='deferred'"):
            _mag_step(table_step=mode, deterministic=True, defer_capacity=8)


# ---- 5. the mirror's deliberate mistakes
def _outcomes(mistake=None):
    out = {}
    for name, make in SCENARIOS.items():
        for pre_forward in (True, False):
            out[name, pre_forward, None] = dc.run_book(make(), mistake, pre_forward)[0].outcome()
    out["main", True, JUMP] = dc.run_book(dc.main(), mistake, True, JUMP)[0].outcome()
    return out


@pytest.mark.parametrize("mistake", dc.MISTAKES)
def test_every_mistake_changes_what_some_scenario_expects(mistake):
    """DESIGN §7q's method on the bookkeeping: a mistake that no scenario can tell from the right books would mean the
    scenarios do not cover it."""
    right, wrong = _outcomes(), _outcomes(mistake)
    found = {key for key in right if right[key] != wrong[key]}
    assert found, f"no scenario tells {mistake} from the right bookkeeping"
    want = {"gap_plus_one": ("past_the_gap", True, None), "gap_minus_one": ("largest_gap", True, None),
            "stale_slot_unchecked": ("main", True, JUMP), "empty_writes_no_history": ("main", True, None),
            "flush_stops_early": ("single_row", True, None), "step_skips_last": ("wrap", False, None)}[mistake]
    assert want in found, (mistake, sorted(map(str, found)))
