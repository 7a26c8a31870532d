"""CPU tests of the dirty-row snapshot and of `fit` over a MagTrainStep: csrc/fit_rows_layout.hpp itself
(tests/native/fit_rows_check.cpp, built with the address and undefined-behaviour sanitizers and run as a program) against
brute force, what is particular to the entry points of csrc/fit_rows_abi.hpp in _native.PRIVATE_ABI (tests/test_host_abi.py
holds the types), their error codes before any GPU work, every refusal of the Python layer before a device call, and the
grid cap the GPU cases were sized for."""
import ctypes
import glob
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import abi_header as ah
import fit_rows_cases as fr
import native_check
import row_mark_cases as rm
from grand_plus_amd import _native
from grand_plus_amd import fit as gfit
from grand_plus_amd import optim_rows as orows
from test_host_mag_det import _mag_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grand_plus_amd", "csrc")
P = ctypes.c_void_p(16)
NAMES = ["gp_fit_rows_mark", "gp_fit_rows_snapshot"]


# ---- 1. the layout header
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = native_check.build(tmp_path_factory, "fit_rows_check")

    def ask(lines):
        return native_check.ints(native_check.run(exe, lines))
    return ask


def test_the_layout_header_reuses_the_bitmap_layout_and_needs_no_hip(tmp_path):
    layout = open(os.path.join(CSRC, "fit_rows_layout.hpp")).read()
    assert re.findall(r"#include\s*[<\"]([^>\"]+)", layout) == ["row_mark_layout.hpp"]
    code = re.sub(r"//[^\n]*", "", layout)
    assert "gp_row_mark::valid_mask(" in code and not re.search(r">>\s*5|&\s*31", code)     # word and bit of a row: not restated
    src = tmp_path / "only_layout.cpp"
    src.write_text('#include "fit_rows_layout.hpp"\nint main() { return (int)gp_fit_rows::grid(9, 2) - 2; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-o", str(tmp_path / "only_layout"), str(src)], check=True,
                   timeout=120)
    subprocess.run([str(tmp_path / "only_layout")], check=True, timeout=60)
    assert fr.WAVES == int(re.search(r"constexpr int kWaves = (\d+);", layout).group(1))


def test_the_grid_cap_is_the_one_the_gpu_cases_were_sized_for():
    hip = open(os.path.join(CSRC, "fit_rows.hip")).read()
    caps = re.findall(r"constexpr int kMaxGrid = (\d+);", hip)
    assert caps == [str(fr.GRID_CAP)], "the cap moved: the second-trip sizes of tests/fit_rows_cases.py must follow"
    assert len(re.findall(r"gp_fit_rows::grid\(n_words, kMaxGrid\)", hip)) == 1
    one_trip = fr.GRID_CAP * fr.WAVES                                # words a full grid owns on one trip
    assert rm.words(fr.V_TWO_TRIPS) == 2 * one_trip and fr.FIRST_TRIP_ROWS == one_trip * 32
    assert one_trip < rm.words(fr.V_PAST_CAP) < 2 * one_trip and fr.V_PAST_CAP % 32


@pytest.mark.parametrize("V", fr.VS + (fr.V_PAST_CAP, fr.V_TWO_TRIPS))
def test_every_word_is_owned_exactly_once(checker, V):
    n_words = rm.words(V)
    for cap in (fr.GRID_CAP, 1, 3):
        ((got_words, grid, waves, trips, lo, hi, past, later),) = checker([f"own {V} {cap}"])
        assert got_words == n_words and grid == min(cap, max(1, -(-n_words // fr.WAVES))) and waves == grid * fr.WAVES
        assert (lo, hi) == (1, 1), f"V={V} cap={cap}: a word is owned {lo} to {hi} times"
        assert trips == -(-n_words // waves) and later == max(0, n_words - waves)
        assert past == waves * trips - n_words < waves                           # only the last trip runs out, once a wave
    if V == fr.V_TWO_TRIPS:
        ((_, grid, waves, trips, _, _, past, later),) = checker([f"own {V} {fr.GRID_CAP}"])
        assert (grid, trips, past, later) == (fr.GRID_CAP, 2, 0, waves)               # every wave goes round exactly twice
    if V == fr.V_PAST_CAP:
        ((_, grid, waves, trips, _, _, _, later),) = checker([f"own {V} {fr.GRID_CAP}"])
        assert (grid, trips, later) == (fr.GRID_CAP, 2, n_words - waves) and 0 < later < waves


@pytest.mark.parametrize("V", fr.VS + (fr.V_PAST_CAP,))
def test_the_copy_of_a_word_is_brute_force(checker, V):
    """Every unit of every set row below V exactly once, nothing of any other row, no row at or above V addressed (the table
    is a heap block of exactly V * per_row counters under the address sanitizer)."""
    n_words = rm.words(V)
    rng = np.random.default_rng(V)
    per_rows = (1, 2, 7, 16, 17, 64, 65, 257) if V < 10 ** 5 else (1, 16)
    for w in sorted({0, n_words - 1, n_words // 2}):
        for word in (0, 1, 0x80000000, 0xFFFFFFFF, 0x80000001, int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 32))):
            want = [32 * w + b for b in range(32) if (word >> b) & 1 and 32 * w + b < V]
            lines = [f"copy {V} {per_row} {w} {word}" for per_row in per_rows]
            for per_row, (g, passes, most, *rows) in zip(per_rows, checker(lines)):
                assert 1 << g >= min(per_row, 64) and (g == 0 or 1 << (g - 1) < per_row) and g <= 6
                assert passes == -(-len(want) // (64 >> g))
                assert rows == want and most == (1 if want else 0), (V, per_row, w, hex(word))
    for r in (0, 31, 32, 33, V - 1):
        (got,) = checker([f"row {r}"])
        assert got == [r >> 5, 1 << (r & 31)]


# ---- 2. the binding
def test_the_table_is_the_headers_prototypes_type_by_type():
    """The generic part -- every type by the convention, the library's exports -- is tests/test_host_abi.py's."""
    protos = ah.prototypes("fit_rows_abi.hpp")
    assert sorted(protos) == sorted(_native.PRIVATE_ABI["fit_rows_abi.hpp"]) == NAMES
    assert [p[2] for p in protos["gp_fit_rows_mark"][1]] == ["device", "d_keys", "n_keys", "n_vocab", "d_dirty", "stream"]
    assert [p[2] for p in protos["gp_fit_rows_snapshot"][1]] == ["device", "d_track", "d_src", "d_dst", "n_vocab", "dim", "d_dirty", "stream"]


def test_the_unit_is_built_and_stays_outside_c_abi_4():
    import __graft_entry__ as entry
    assert "fit_rows.hip" in entry.LIB_UNITS and os.path.exists(os.path.join(CSRC, "fit_rows.hip"))
    for hdr in ("fit_rows_abi.hpp", "fit_rows_layout.hpp", "row_mark_layout.hpp"):
        assert os.path.join(CSRC, hdr) in entry.lib_sources()
    public = "".join(open(p).read() for p in glob.glob(os.path.join(ROOT, "include", "*.h")))
    assert "fit_rows" not in public
    assert _native.lib().gp_abi_version() == 4
    hip = open(os.path.join(CSRC, "fit_rows.hip")).read()
    for hdr in ("gp_common.hpp", "fit_rows_layout.hpp", "fit_rows_abi.hpp"):
        assert f'#include "{hdr}"' in hip
    code = re.sub(r"//[^\n]*", "", hip)
    assert re.findall(r"atomic\w*", code) == ["atomicOr"]                           # one atomic, the OR of the mark kernel
    assert not re.search(r"\basm\b|printf|\bassert\s*\(|__builtin_amdgcn_|hipMemcpy|hipMalloc|Synchronize", code)
    for call in ("gp_row_mark::word_of(", "gp_row_mark::bit_of(", "gp_row_mark::words(", "gp_fit_rows::owned_word(", "gp_fit_rows::trips(",
                 "gp_fit_rows::live_bits(", "gp_fit_rows::lane_slot(", "gp_fit_rows::lane_first(", "gp_fit_rows::nth_row(",
                 "gp_fit_rows::passes(", "gp_fit_rows::group_log2(", "gp_fit_rows::grid("):
        assert call in code, call
    # fit.hip is what it was: the snapshot of whole tensors and the constants tests/second_trip_cases.py reads
    assert "fit_rows" not in open(os.path.join(CSRC, "fit.hip")).read()


# ---- 3. error codes
def test_the_entries_return_their_error_codes_before_any_gpu_work():
    """No device pointer here is real: every call has to stop at its argument checks."""
    E, N, OK = _native.GP_ERR_INVALID_ARG, _native.GP_ERR_NULL, _native.GP_OK
    L = _native.lib()
    odd = ctypes.c_void_p(18)

    def mark(keys=P, n_keys=5, V=50, dirty=P):
        return L.gp_fit_rows_mark(0, keys, n_keys, V, dirty, None)

    for kw in (dict(V=0), dict(V=-2), dict(n_keys=-1), dict(keys=odd), dict(dirty=odd)):
        assert mark(**kw) == E, kw
    assert "gp_fit_rows_mark" in L.gp_last_error().decode()
    for name in ("keys", "dirty"):
        assert mark(**{name: None}) == N, name
    assert mark(keys=None, V=0) == E                                              # sizes are judged first
    assert mark(n_keys=0) == OK                                                   # nothing to mark: nothing launched
    assert mark(n_keys=0, keys=None) == N and mark(n_keys=0, V=0) == E            # an empty list is still checked

    def snap(track=P, src=P, dst=P, V=50, dim=7, dirty=P):
        return L.gp_fit_rows_snapshot(0, track, src, dst, V, dim, dirty, None)

    for kw in (dict(V=0), dict(V=-1), dict(dim=0), dict(dim=-3), dict(V=2 ** 62, dim=4), dict(V=2 ** 61, dim=4), dict(track=odd),
               dict(src=odd), dict(dst=odd), dict(dirty=odd)):
        assert snap(**kw) == E, kw
    assert "gp_fit_rows_snapshot" in L.gp_last_error().decode()
    for name in ("track", "src", "dst", "dirty"):
        assert snap(**{name: None}) == N, name
    assert snap(src=None, dim=0) == E
    assert snap(V=2 ** 61 - 1, dim=4, dst=None) == N                              # 2^63 - 4 words pass the size check


# ---- 4. the Python layer
class _Cuda(torch.Tensor):
    """A CPU tensor that says it is on the GPU: it passes the type checks of the Python layer, which must refuse before it
    reaches the library."""
    @property
    def is_cuda(self):
        return True


def _no_device(monkeypatch):
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the native library was reached"))


def test_dirty_rows_needs_the_lazy_table_step(monkeypatch):
    from grand_plus_amd import MagTrainStep
    _no_device(monkeypatch)
    assert inspect.signature(MagTrainStep.__init__).parameters["dirty_rows"].default is False
    for kw in (dict(deterministic=True), dict(deterministic=False), dict(table_step="exact", deterministic=True),
               dict(table_step="exact", row_list="bitmap", deterministic=False)):
        with pytest.raises(ValueError, match="dirty_rows=True needs table_step='lazy'"):
            _mag_step(dirty_rows=True, **kw)
    for kw in (dict(deterministic=True), dict(row_list="bitmap", deterministic=False)):   # everything passes: only the device is missing
        with pytest.raises(ValueError, match="no CPU fallback"):
            _mag_step(dirty_rows=True, table_step="lazy", **kw)
    with pytest.raises(ValueError, match="no CPU fallback"):
        _mag_step()                                                               # the default builds what it built before


def test_track_dirty_makes_the_bitmap_once_and_the_default_marks_nothing(monkeypatch):
    _no_device(monkeypatch)
    for cls in (orows.RowGrad, orows.BitmapRowGrad):
        for V in (1, 32, 33, 4097):
            rg = cls(torch.zeros(V, 3).as_subclass(_Cuda))
            assert rg.dirty is None
            rg.fill(torch.full((1,), V, dtype=torch.int64))                       # no bitmap: no launch, as before
            d = rg.track_dirty()
            assert d is rg.dirty and d.dtype == torch.int32 and d.shape == (rm.words(V),) and not d.any()
            assert rg.track_dirty() is d                                          # made once: graphs hold its address
    rg = orows.RowGrad(torch.zeros(5, 3).as_subclass(_Cuda))
    rg.track_dirty()
    with pytest.raises(BaseException, match="the native library was reached"):    # with a bitmap, fill marks
        rg.fill(torch.full((1,), 5, dtype=torch.int64))


def test_the_tracker_refuses_a_row_grad_before_any_device_call(monkeypatch):
    from grand_plus_amd.mlp import MagMLP
    _no_device(monkeypatch)
    assert inspect.signature(gfit.BestTracker.__init__).parameters["row_grad"].kind is inspect.Parameter.KEYWORD_ONLY
    model = MagMLP(9, 3, 4, 2, True, 0.0, 0.5, True)
    rg = orows.RowGrad(model.embeds.weight.detach().as_subclass(_Cuda))
    with pytest.raises(ValueError, match=r"track_dirty\(\)"):
        gfit.BestTracker(model, "cuda:0", row_grad=rg)                            # no bitmap
    with pytest.raises(ValueError, match=r"track_dirty\(\)"):
        gfit.BestTracker(model, "cuda:0", row_grad=object())
    rg.track_dirty()
    other = orows.RowGrad(torch.zeros(9, 4).as_subclass(_Cuda))
    other.track_dirty()
    with pytest.raises(ValueError, match="not in model.state_dict"):
        gfit.BestTracker(model, "cuda:0", row_grad=other)
    with pytest.raises(ValueError, match="stop_mode"):
        gfit.BestTracker(model, "cuda:0", "loss", row_grad=rg)
    with pytest.raises(ValueError, match="is on cpu"):                            # the row_grad passes: only the device is missing
        gfit.BestTracker(model, "cuda:0", row_grad=rg)


def test_a_bad_valid_batch_is_refused_before_any_device_call(monkeypatch):
    from grand_plus_amd import MagTrainStep, TrainStep
    _no_device(monkeypatch)
    for f in (gfit.fit, gfit.FitLoop.__init__):
        p = inspect.signature(f).parameters["valid_batch"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert TrainStep._valid_batch is None and MagTrainStep._valid_batch == 100
    s = gfit.Sampler(3, 3, 2, 2)
    for cls in (TrainStep, MagTrainStep):
        step = object.__new__(cls)                                                # nothing of it may be touched
        for bad in (0, -1, 2.0, True, "100", 2 ** 31):
            with pytest.raises(ValueError, match="valid_batch must be None or an int"):
                gfit.FitLoop(step, s, [0], valid_batch=bad)
            with pytest.raises(ValueError, match="valid_batch must be None or an int"):
                gfit.fit(step, s, [0], epochs=1, valid_batch=bad)
    with pytest.raises(TypeError, match="fit takes a TrainStep"):
        gfit.fit(object(), s, [0], epochs=1)


def test_the_new_names_are_exported():
    import grand_plus_amd
    from grand_plus_amd import mag
    assert grand_plus_amd.valid_mag_plan is mag.valid_mag_plan and grand_plus_amd.valid_mag_pass is mag.valid_mag_pass
    assert "valid_mag_plan" not in grand_plus_amd.__all__
    assert list(inspect.signature(mag.valid_mag).parameters) == ["model", "rows", "attr_indptr", "attr_indices", "attr_data", "idx_val",
                                                                 "labels", "batch_size", "dropnode_rate", "return_counts"]
    assert mag.ValidMagPlan._fields == ("model", "rows", "attr", "labels", "idx", "pos", "buf", "batch_size")   # nothing of the weights
    with pytest.raises(TypeError, match="valid_mag: model must be a MagMLP"):
        mag.valid_mag_plan(object(), None, None, None, None, [0], None)


# ---- 5. the mirror
@pytest.mark.parametrize("V", fr.VS)
def test_the_mirror_marks_and_copies_by_brute_force(V):
    for name, keys in fr.key_lists(V).items():
        got = fr.mark(fr.foreign(V), keys, V)
        want = set(rm.rows_of(fr.foreign(V), V).tolist()) | {int(k) for k in keys if 0 <= k < V}
        assert rm.rows_of(got, V).tolist() == sorted(want), name
        assert not (got[-1] & np.uint32(~rm.valid_mask(rm.words(V) - 1, V) & 0xFFFFFFFF))
    lists = fr.key_lists(V)
    assert len(lists["empty"]) == 0 and (lists["sentinels"] == V).all() and (lists["strays"] < 0).any() and (lists["strays"] > V).any()
    src, dst = fr.tables(V, 7)
    for name, bm in fr.bitmaps(V).items():
        out, after = fr.snapshot(1, src, dst, bm, V)
        rows = rm.rows_of(bm, V)
        for r in range(V):
            assert np.array_equal(out[r], src[r] if r in rows else dst[r]), (name, r)
        assert not after.any()
        out, after = fr.snapshot(0, src, dst, bm, V)
        assert np.array_equal(out, dst) and np.array_equal(after, bm)
