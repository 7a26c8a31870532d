"""CPU tests of the atomic backward's row list: csrc/row_mark_layout.hpp itself (tests/native/row_mark_check.cpp,
built with the address and undefined-behaviour sanitizers and run as a program) against brute force, what is particular to the
entry points of csrc/row_mark_abi.hpp in _native.PRIVATE_ABI (tests/test_host_abi.py holds the types), their error codes
before any GPU work, every refusal of the Python layer before a device call, and the numpy mirror's deliberate mistakes."""
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
import mag_cases as mc
import native_check
import row_mark_cases as rm
from grand_plus_amd import _native
from grand_plus_amd import optim_rows as orows
from test_host_mag_det import _mag_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grand_plus_amd", "csrc")
P = ctypes.c_void_p(16)
NAMES = ["gp_row_list_compact", "gp_row_list_zero", "gp_row_mark_mag"]


# ---- 1. the layout header
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = native_check.build(tmp_path_factory, "row_mark_check")

    def ask(lines):
        return native_check.ints(native_check.run(exe, lines))
    return ask


def test_the_layout_header_needs_nothing_but_the_standard_library(tmp_path):
    layout = open(os.path.join(CSRC, "row_mark_layout.hpp")).read()
    assert re.findall(r"#include\s*[<\"]([^>\"]+)", layout) == ["cstdint"]
    src = tmp_path / "only_layout.cpp"
    src.write_text('#include "row_mark_layout.hpp"\nint main() { return (int)gp_row_mark::words(33) - 2; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-o", str(tmp_path / "only_layout"), str(src)], check=True,
                   timeout=120)
    subprocess.run([str(tmp_path / "only_layout")], check=True, timeout=60)
    assert rm.TILE == int(re.search(r"constexpr int kTile = (\d+);", layout).group(1))
    assert rm.MAX_CHUNKS == int(re.search(r"constexpr int kMaxChunks = (\d+);", layout).group(1)) == orows.ROW_LIST_PARTIALS
    stage = open(os.path.join(CSRC, "mag_stage.hpp")).read()
    assert rm.GRID_CAP == int(re.search(r"constexpr int kGridCap = (\d+);", stage).group(1))


@pytest.mark.parametrize("V", rm.VS + (rm.V_CHUNKS,))
def test_the_compaction_is_brute_force(checker, V):
    """Every bitmap of the grid -- empty, full, the single bit at row 0 and at row V - 1, a random third, stray bits at or
    above V -- at the capacities total - 1, total and total + 1, from the header under the sanitizers: the keys, the total,
    the overflow, the tail and the chunks' partial counts."""
    n_words = rm.words(V)
    for name, bm in rm.bitmaps(V).items():
        rows = rm.rows_of(bm, V)
        assert len(rows) == {"empty": 0, "empty_stray": 0, "full": V, "full_stray": V, "row0": 1, "last": 1}.get(name, len(rows))
        for cap in rm.capacities(len(rows)):
            keys, (total, over, tail, got_words, got_chunks), partials = checker([f"compact {V} {cap} " + " ".join(map(str, bm))])
            want, want_total, want_over, _ = rm.compact(bm, V, cap)
            assert keys == want[:cap].tolist(), (name, cap)
            assert (total, bool(over), tail) == (want_total, want_over, min(want_total, cap)) and total == len(rows), (name, cap)
            assert keys[:tail] == rows[:tail].tolist() and keys[tail:] == [V] * (cap - tail), (name, cap)
            assert (got_words, got_chunks) == (n_words, rm.chunks(n_words)) and sum(partials) == total
            walked = rm.compact(bm, V, cap, slow=True)
            assert (walked[0] == want).all() and walked[1:3] == (want_total, want_over) and not walked[3].any()


def test_words_bits_and_chunks(checker):
    for r in (0, 1, 31, 32, 33, 63, 64, 4096, 2 ** 31 - 1, 2 ** 31, 2 ** 40 + 37):
        (got,) = checker([f"row {r}"])
        assert got == [r >> 5, 1 << (r & 31)]
    for n_words in (0, 1, 255, 256, 257, 769, rm.MAX_CHUNKS * rm.TILE, rm.MAX_CHUNKS * rm.TILE + 1, rm.words(rm.V_TILES), 10 ** 7):
        (got,) = checker([f"chunks {n_words}"])
        n, per, begins = got[0], got[1], got[2:]
        assert n == rm.chunks(n_words) and 1 <= n <= rm.MAX_CHUNKS and per == rm.chunk_words(n_words, n) and per % rm.TILE == 0
        assert begins == [rm.chunk_begin(c, n_words, n) for c in range(n + 1)]
        assert begins[0] == 0 and begins[-1] == n_words and all(a <= b for a, b in zip(begins, begins[1:]))   # contiguous, ascending, all
    assert rm.chunks(rm.words(rm.V_CHUNKS)) == 4 and rm.chunk_words(rm.words(rm.V_CHUNKS), 4) == rm.TILE
    assert rm.chunks(rm.words(rm.V_TILES)) == rm.MAX_CHUNKS and rm.chunk_words(rm.words(rm.V_TILES), rm.MAX_CHUNKS) == 2 * rm.TILE


# ---- 2. the binding
def test_the_table_is_the_headers_prototypes_type_by_type():
    """The generic part -- every type by the convention, the library's exports -- is tests/test_host_abi.py's."""
    protos, code = ah.prototypes("row_mark_abi.hpp"), ah.read("row_mark_abi.hpp")[1]
    assert sorted(protos) == sorted(_native.PRIVATE_ABI["row_mark_abi.hpp"]) == NAMES
    # the mark takes gp_mag_det_keys' operands up to n_batch, name by name
    text = open(os.path.join(CSRC, "mag_det_abi.hpp")).read()
    det = re.search(r"int gp_mag_det_keys\(([^)]*)\)", text).group(1)
    det_names = [p.split()[-1].lstrip("*") for p in det.split(",")]
    assert [p[2] for p in protos["gp_row_mark_mag"][1][:11]] == det_names[:11] and det_names[10] == "n_batch"
    assert int(re.search(r"#define GP_ROW_LIST_PARTIALS (\d+)", code).group(1)) == orows.ROW_LIST_PARTIALS


def test_the_entry_points_stay_outside_c_abi_4_and_share_the_slot_rule():
    import __graft_entry__ as entry
    assert "row_mark.hip" in entry.LIB_UNITS
    for hdr in ("row_mark_abi.hpp", "row_mark_layout.hpp", "mag_stage.hpp"):
        assert os.path.join(CSRC, hdr) in entry.lib_sources()
    public = "".join(open(p).read() for p in glob.glob(os.path.join(ROOT, "include", "*.h")))
    assert "row_mark" not in public and "row_list" not in public and "ROW_LIST" not in public
    assert _native.lib().gp_abi_version() == 4
    hip = open(os.path.join(CSRC, "row_mark.hip")).read()
    for hdr in ("mag_stage.hpp", "row_mark_layout.hpp", "row_mark_abi.hpp"):
        assert f'#include "{hdr}"' in hip
    code = re.sub(r"//[^\n]*", "", hip)
    # one atomic, the OR of the mark kernel; nothing that reads the host or debugs
    assert re.findall(r"atomic\w*", code) == ["atomicOr"]
    assert not re.search(r"\basm\b|printf|\bassert\s*\(|__builtin_amdgcn_s_|hipMemcpy|hipMalloc|Synchronize", code)
    for call in ("slot_node(", "gp_row_mark::word_of(", "gp_row_mark::bit_of(", "gp_row_mark::valid_mask(", "gp_row_mark::chunk_begin(",
                 "gp_row_mark::emit_word(", "gp_row_mark::tail_begin(", "gp_row_mark::overflowed(", "gp_row_mark::chunks(", "kGridCap"):
        assert call in code, call
    # the slot rule is stated once, in the header both units include
    for name in ("struct SlotArgs", "bool slot_node("):
        holders = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*")) if name in open(p, errors="replace").read())
        assert holders == ["mag_stage.hpp"], (name, holders)


# ---- 3. error codes
def test_the_entries_return_their_error_codes_before_any_gpu_work():
    """No device pointer here is real: every call has to stop at its argument checks."""
    E, N, OK = _native.GP_ERR_INVALID_ARG, _native.GP_ERR_NULL, _native.GP_OK
    L = _native.lib()

    def mark(V=50, indptr=P, indices=P, n_nodes=12, col=P, filled=P, n_rows=6, K=5, batch=P, B=4, bitmap=P):
        return L.gp_row_mark_mag(0, V, indptr, indices, n_nodes, col, filled, n_rows, K, batch, B, bitmap, None)

    for kw in (dict(V=0), dict(V=-2), dict(n_nodes=-1), dict(n_rows=-1), dict(K=0), dict(K=1025), dict(B=-1), dict(B=2 ** 31 - 1, K=2),
               dict(B=2 ** 21, K=1024)):
        assert mark(**kw) == E, kw
    assert "gp_row_mark_mag" in L.gp_last_error().decode()
    for name in ("indptr", "indices", "col", "bitmap"):
        assert mark(**{name: None}) == N, name
    assert mark(indptr=None, K=0) == E                                            # sizes are judged first
    assert mark(B=0) == OK and mark(B=0, filled=None, batch=None) == OK           # nothing to mark: nothing launched
    assert mark(B=2 ** 21 - 1, K=1024, bitmap=None) == N                          # 2^31 - 1024 slots pass the size check

    def compact(V=50, bitmap=P, cap=10, keys=P, count=P, partials=P, flag=P):
        return L.gp_row_list_compact(0, V, bitmap, cap, keys, count, partials, flag, None)

    for kw in (dict(V=0), dict(V=-1), dict(cap=0), dict(cap=-4)):
        assert compact(**kw) == E, kw
    assert "gp_row_list_compact" in L.gp_last_error().decode()
    for name in ("bitmap", "keys", "count", "partials", "flag"):
        assert compact(**{name: None}) == N, name
    assert compact(keys=None, cap=0) == E

    def zero(keys=P, cap=10, V=50, H=7, values=P):
        return L.gp_row_list_zero(0, keys, cap, V, H, values, None)

    for kw in (dict(cap=0), dict(cap=-1), dict(V=0), dict(H=0), dict(H=-3), dict(V=2 ** 62, H=4)):
        assert zero(**kw) == E, kw
    assert "gp_row_list_zero" in L.gp_last_error().decode()
    for name in ("keys", "values"):
        assert zero(**{name: None}) == N, name
    assert zero(values=None, H=0) == E


# ---- 4. the Python layer
class _Cuda(torch.Tensor):
    """A CPU tensor that says it is on the GPU: it passes the type checks of the Python layer, which must refuse before it
    reaches the library."""
    @property
    def is_cuda(self):
        return True


def _fake(t):
    return None if t is None else t.as_subclass(_Cuda)


def _no_device(monkeypatch):
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the native library was reached"))


def test_bitmap_row_grad_is_a_row_grad_with_a_bitmap(monkeypatch):
    _no_device(monkeypatch)
    import grand_plus_amd
    assert issubclass(orows.BitmapRowGrad, orows.RowGrad) and "BitmapRowGrad" in orows.__all__
    assert grand_plus_amd.BitmapRowGrad is orows.BitmapRowGrad and "BitmapRowGrad" not in grand_plus_amd.__all__
    with pytest.raises(TypeError, match="dense contiguous float32"):
        orows.BitmapRowGrad(torch.zeros(3, 4, dtype=torch.float64))
    with pytest.raises(TypeError, match="no CPU fallback"):
        orows.BitmapRowGrad(torch.zeros(4, 3))
    for V in (1, 32, 33, 4097):
        rg = orows.BitmapRowGrad(_fake(torch.zeros(V, 3)))
        assert rg.bitmap.dtype == torch.int32 and rg.bitmap.shape == (rm.words(V),) and not rg.bitmap.any()
        assert rg.count.dtype == torch.int64 and rg.count.shape == (1,)
        assert rg.partials.dtype == torch.int64 and rg.partials.shape == (orows.ROW_LIST_PARTIALS,)
        assert rg.values.shape == (V, 3) and rg.keys is None and not rg.filled()
        at = rg.bitmap.data_ptr()
        rg.bitmap.fill_(-1)
        rg.reset()
        assert not rg.bitmap.any() and rg.bitmap.data_ptr() == at                   # zeroed in place: graphs hold its address


def test_mag_prop_rows_refuses_a_bitmap_row_grad_before_any_device_call(monkeypatch):
    from grand_plus_amd.mag import mag_prop_rows
    _no_device(monkeypatch)
    Pm = mc.case("h7_k5_s3")["P"]
    a = dict(attr_indptr=Pm.indptr, attr_indices=Pm.indices, attr_data=Pm.data, col=Pm.col.reshape(-1), val=Pm.val.reshape(-1),
             filled=Pm.filled)
    a = {k: _fake(v) for k, v in a.items()}
    w = _fake(Pm.W.clone().requires_grad_(True))
    brg = orows.BitmapRowGrad(w)
    with pytest.raises(ValueError, match=r"BitmapRowGrad is the atomic backward's.*plain optim_rows\.RowGrad"):
        mag_prop_rows(w, **a, K=Pm.K, deterministic=True, max_entries=100, row_grad=brg)
    torch.use_deterministic_algorithms(True)
    try:
        with pytest.raises(ValueError, match=r"BitmapRowGrad is the atomic backward's.*plain optim_rows\.RowGrad"):
            mag_prop_rows(w, **a, K=Pm.K, max_entries=100, row_grad=brg)         # torch's flag decides
    finally:
        torch.use_deterministic_algorithms(False)
    for kw in (dict(deterministic=False), dict()):
        with pytest.raises(ValueError, match="BitmapRowGrad needs max_entries="):
            mag_prop_rows(w, **a, K=Pm.K, row_grad=brg, **kw)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="max_entries must be an int >= 1"):
            mag_prop_rows(w, **a, K=Pm.K, deterministic=False, max_entries=bad, row_grad=brg)
    other = _fake(Pm.W.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="made for another tensor"):
        mag_prop_rows(other, **a, K=Pm.K, deterministic=False, max_entries=100, row_grad=brg)
    for bad in (torch.zeros(1, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), [0]):
        with pytest.raises(TypeError, match="overflow must be a contiguous int32 tensor of one element"):
            mag_prop_rows(w, **a, K=Pm.K, deterministic=False, max_entries=100, row_grad=brg, overflow=bad)
    # a plain RowGrad in the atomic mode keeps its refusal, word for word
    rg = orows.RowGrad(w)
    want = ("row_grad needs the deterministic backward: deterministic=True (or torch's deterministic mode) and "
            "max_entries=; the atomic backward keeps no list of the rows it touched (DESIGN §9)")
    for kw in (dict(deterministic=False, max_entries=100), dict(max_entries=100), dict(deterministic=True)):
        with pytest.raises(ValueError) as e:
            mag_prop_rows(w, **a, K=Pm.K, row_grad=rg, **kw)
        assert str(e.value) == want


def test_mag_train_step_refuses_a_row_list_before_any_device_call(monkeypatch):
    from grand_plus_amd import MagTrainStep
    _no_device(monkeypatch)
    assert inspect.signature(MagTrainStep.__init__).parameters["row_list"].default is None
    for bad in ("sort", "Bitmap", 1, True):
        with pytest.raises(ValueError, match="row_list must be None or 'bitmap'"):
            _mag_step(row_list=bad, table_step="lazy", deterministic=False)
    with pytest.raises(ValueError, match="row_list='bitmap' needs a table_step"):
        _mag_step(row_list="bitmap", deterministic=False)
    with pytest.raises(ValueError, match="'exact' or 'lazy'"):
        _mag_step(row_list="bitmap", table_step="dense", deterministic=False)
    for mode in ("exact", "lazy"):
        with pytest.raises(ValueError, match="needs deterministic=False"):
            _mag_step(row_list="bitmap", table_step=mode, deterministic=True)
        torch.use_deterministic_algorithms(True)
        try:
            with pytest.raises(ValueError, match="needs deterministic=False"):
                _mag_step(row_list="bitmap", table_step=mode)                       # torch's flag is on
        finally:
            torch.use_deterministic_algorithms(False)
        # None keeps today's refusal of a table step over the atomic backward
        with pytest.raises(ValueError, match="needs the deterministic table gradient"):
            _mag_step(table_step=mode, deterministic=False)
        for kw in (dict(deterministic=False), dict()):                               # everything passes: only the device is missing
            with pytest.raises(ValueError, match="no CPU fallback"):
                _mag_step(row_list="bitmap", table_step=mode, **kw)


# ---- 5. the mirror's deliberate mistakes
def _compaction_cases():
    for V in rm.VS + (rm.V_CHUNKS,):
        for name, bm in rm.bitmaps(V).items():
            for cap in rm.capacities(len(rm.rows_of(bm, V))):
                yield f"V{V}-{name}-cap{cap}", bm, V, cap
    # two chunks that each hold more rows than the capacity
    V = rm.V_CHUNKS
    yield "chunks-cap2", rm.bitmap_of(V, [3, 4, 5, 9000, 9001, 9002]), V, 2


def _mark_cases():
    for name in ("h7_k5_s3", "h64_k32_s2"):
        c = mc.case(name)
        Pm = c["P"]
        for batch in (None, c["batch"]):
            B = Pm.S_rows if batch is None else len(batch)
            kept = np.zeros(B * Pm.K, dtype=bool)                                   # DropNode dropped every slot
            yield f"{name}-{'all' if batch is None else 'batch'}", Pm, batch, kept


@pytest.mark.parametrize("mistake", rm.MISTAKES)
def test_every_mistake_changes_what_some_case_expects(mistake):
    """DESIGN §7q's method on the row list: a mistake that no case of the grid can tell from the right answer would mean the
    grid does not cover it."""
    found = []
    if mistake == "dropped_slot_not_marked":
        for name, Pm, batch, kept in _mark_cases():
            right = rm.marked_rows(Pm, batch, kept)
            assert len(right) and (np.diff(right) > 0).all()
            if not np.array_equal(right, rm.marked_rows(Pm, batch, kept, mistake)):
                found.append(name)
    else:
        for name, bm, V, cap in _compaction_cases():
            right, wrong = rm.compact(bm, V, cap), rm.compact(bm, V, cap, mistake)
            if not (np.array_equal(right[0], wrong[0]) and right[1:3] == wrong[1:3] and np.array_equal(right[3], wrong[3])):
                found.append(name)
    assert found, f"no case of the grid tells {mistake} from the right answer"
    want = {"last_partial_word_dropped": "V33-", "bit_above_v_emitted": "_stray", "offset_from_wrong_partial": f"V{rm.V_CHUNKS}-",
            "truncated_per_chunk": "chunks-cap2"}.get(mistake)
    if want:
        assert any(want in name for name in found), found
    if mistake in ("offset_from_wrong_partial", "truncated_per_chunk"):               # only several chunks can tell
        assert all(name.startswith(f"V{rm.V_CHUNKS}-") or name == "chunks-cap2" for name in found), found
