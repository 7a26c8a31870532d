"""The two kernels of the dirty-row snapshot (csrc/fit_rows.hip) on the GPU, bitwise against the numpy mirror of
tests/fit_rows_cases.py.  Every buffer lies between guard bands that nothing may write, and both launches run with host
synchronisation an error."""
import ctypes

import numpy as np
import pytest
import torch

import fit_rows_cases as fr
import row_mark_cases as rm

pytestmark = pytest.mark.gpu

G = 16                        # guard words on either side of a buffer
GUARD_BITS = 0x6A6A6A6A


class _Words:
    """A device buffer of 32-bit words holding `a` (uint32, any shape) between two guard bands, `offset` words into a
    16-byte aligned block."""

    def __init__(self, a, offset=0):
        a = np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)
        self.n, self.at = a.size, G + offset
        self.full = torch.full((a.size + 2 * G + offset,), GUARD_BITS, dtype=torch.int32, device="cuda")
        assert self.full.data_ptr() % 16 == 0
        self.set(a)

    def ptr(self):
        return self.full.data_ptr() + 4 * self.at

    def set(self, a):
        a = np.array(a, dtype=np.uint32).reshape(-1)                                # a writable copy: the cases are read-only
        self.full[self.at:self.at + self.n].copy_(torch.from_numpy(a.view(np.int32)))

    def get(self):
        full = self.full.cpu().numpy().view(np.uint32)
        assert (full[:self.at] == GUARD_BITS).all() and (full[self.at + self.n:] == GUARD_BITS).all(), "a guard band was written"
        return full[self.at:self.at + self.n].copy()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _no_sync(call):
    """`call()` with host synchronisation an error; the code is loaded by then (every test's first launch is outside)."""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        rc = call()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    return rc


@pytest.fixture(scope="module", autouse=True)
def loaded():
    """One launch of either kernel before any test: loading the code object may synchronise, the kernels may not."""
    from grand_plus_amd import _native
    L = _native.lib()
    keys = torch.zeros(1, dtype=torch.int64, device="cuda")
    dirty = torch.zeros(1, dtype=torch.int32, device="cuda")
    track = torch.zeros(5, dtype=torch.int64, device="cuda")
    _native.raise_for_status(L.gp_fit_rows_mark(0, keys.data_ptr(), 1, 1, dirty.data_ptr(), _stream()))
    _native.raise_for_status(L.gp_fit_rows_snapshot(0, track.data_ptr(), keys.data_ptr(), keys.data_ptr(), 1, 1, dirty.data_ptr(), _stream()))
    torch.cuda.synchronize()


def _track(copy_now):
    from grand_plus_amd.fit import GpFitTrack
    image = GpFitTrack(best_loss=1.5, best_acc=0.25, best_tick=7, copy_now=copy_now)
    return bytes(image), torch.frombuffer(bytearray(bytes(image)), dtype=torch.int64).cuda()


# ---- the mark
def _mark(V, keys, before):
    from grand_plus_amd import _native
    L = _native.lib()
    dirty = _Words(before)
    k = torch.full((len(keys) + 2 * G,), 3 % V, dtype=torch.int64, device="cuda")   # the guards name a real row: read, they would mark
    k[G:G + len(keys)].copy_(torch.from_numpy(np.asarray(keys, np.int64)))
    rc = _no_sync(lambda: L.gp_fit_rows_mark(0, k.data_ptr() + 8 * G, len(keys), V, dirty.ptr(), _stream()))
    _native.raise_for_status(rc)
    return dirty.get()


@pytest.mark.parametrize("V", fr.VS)
def test_the_mark_sets_the_lists_rows_and_keeps_foreign_bits(V):
    empty = np.zeros(rm.words(V), np.uint32)
    for name, keys in fr.key_lists(V).items():
        for label, before in (("zeros", empty), ("foreign", fr.foreign(V))):
            got = _mark(V, keys, before)
            want = fr.mark(before, keys, V)
            assert np.array_equal(got, want), f"V={V} {name} over {label}: the bitmap is not the mirror's"
            assert np.array_equal(got & before, before), f"V={V} {name}: a bit that was set is gone"
            assert np.array_equal(_mark(V, keys, before), got), f"V={V} {name}: two runs differ"
        if name in ("empty", "sentinels"):
            assert np.array_equal(_mark(V, keys, empty), empty)


def test_more_keys_than_the_grid_has_threads():
    """2 048 workgroups of 256 threads: with more than twice as many keys every thread goes round its loop, and rows that
    only the third trip names tell."""
    V = 4097
    n = 2 * fr.GRID_CAP * 256 + 300
    keys = np.sort(np.concatenate([np.arange(n - 300) % 1000, 3000 + np.arange(300)])).astype(np.int64)
    assert (keys[-300:] >= 3000).all() and keys[-301] < 1000
    got = _mark(V, keys, np.zeros(rm.words(V), np.uint32))
    assert np.array_equal(rm.rows_of(got, V), np.concatenate([np.arange(1000), 3000 + np.arange(300)]))


# ---- the snapshot
def _snapshot(V, dim, bm, copy_now, offset=0, tables=None):
    """gp_fit_rows_snapshot from the mirror's tables, both `offset` words into a 16-byte aligned block: (the destination,
    the bitmap) afterwards as uint32."""
    from grand_plus_amd import _native
    L = _native.lib()
    src, dst = tables if tables is not None else fr.tables(V, dim)
    s, d, dirty = _Words(src, offset), _Words(dst, offset), _Words(bm)
    assert (s.ptr() % 16 == 0) == (offset % 4 == 0) and (d.ptr() % 16 == 0) == (offset % 4 == 0)
    image, track = _track(copy_now)
    rc = _no_sync(lambda: L.gp_fit_rows_snapshot(0, track.data_ptr(), s.ptr(), d.ptr(), V, dim, dirty.ptr(), _stream()))
    _native.raise_for_status(rc)
    assert np.array_equal(s.get(), np.asarray(src).reshape(-1)), "the source was written"
    assert track.cpu().numpy().tobytes() == image, "the track was written"
    return d.get().reshape(V, dim), dirty.get()


@pytest.mark.parametrize("dim", fr.DIMS)
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "unaligned"])
def test_dirty_rows_are_copied_bit_for_bit_and_every_other_row_keeps_its_pattern(dim, offset):
    for V in (33, 4097) if dim in (7, 64) else (33,):
        src, dst = fr.tables(V, dim)
        assert (src == fr.NAN_BITS).any() and (src == fr.NEG_ZERO).any()
        for name, bm in fr.bitmaps(V).items():
            rows = rm.rows_of(bm, V)
            got, after = _snapshot(V, dim, bm, 1, offset)
            want, want_after = fr.snapshot(1, src, dst, bm, V)
            clean = np.ones(V, bool)
            clean[rows] = False
            assert np.array_equal(got[rows], src[rows]), f"V={V} dim={dim} {name}: a dirty row is not the source's bits"
            assert np.array_equal(got[clean], dst[clean]), f"V={V} dim={dim} {name}: a clean row lost its pattern"
            assert np.array_equal(got, want) and not after.any() and np.array_equal(after, want_after), f"V={V} dim={dim} {name}"
            # copy_now = 0: the destination and the bitmap keep every bit
            got, after = _snapshot(V, dim, bm, 0, offset)
            assert np.array_equal(got, dst) and np.array_equal(after, bm), f"V={V} dim={dim} {name}: copy_now = 0 wrote"


@pytest.mark.parametrize("V", fr.VS)
def test_every_vocabulary_edge_and_the_single_bits(V):
    src, dst = fr.tables(V, 7)
    names = set(fr.bitmaps(V))
    assert {"empty", "full", "row0", f"row{V - 1}", "full_stray", "stray_alone"} <= names and (V <= 31 or "row31" in names)
    for name, bm in fr.bitmaps(V).items():
        got, after = _snapshot(V, 7, bm, 1)
        want, _ = fr.snapshot(1, src, dst, bm, V)
        assert np.array_equal(got, want) and not after.any(), f"V={V} {name}"


def test_every_wave_goes_round_its_loop_twice():
    """dim = 1 and 2 * 2 048 * 4 words: the second half of the rows is reached on the second trip alone, and is compared on
    its own first."""
    V = fr.V_TWO_TRIPS
    rng = np.random.default_rng(5)
    src = rng.integers(1, 2 ** 31, (V, 1), dtype=np.int64).astype(np.uint32)
    dst = np.zeros((V, 1), np.uint32)
    rows = np.unique(np.concatenate([rng.integers(0, V, V // 3), [0, fr.FIRST_TRIP_ROWS - 1, fr.FIRST_TRIP_ROWS, V - 1]]))
    bm = rm.bitmap_of(V, rows)
    got, after = _snapshot(V, 1, bm, 1, tables=(src, dst))
    want, _ = fr.snapshot(1, src, dst, bm, V)
    second = slice(fr.FIRST_TRIP_ROWS, V)
    assert (rows >= fr.FIRST_TRIP_ROWS).sum() > 1000
    assert np.array_equal(got[second], want[second]), "the rows of the second trip differ"
    assert not after[fr.FIRST_TRIP_ROWS // 32:].any(), "a word of the second trip was not cleared"
    assert np.array_equal(got, want) and not after.any()


def test_mark_then_snapshot_is_what_the_tracker_issues():
    """The two entry points back to back on one stream, as RowGrad.fill and BestTracker.update issue them: marks accumulate
    over two lists, one snapshot copies their union, a second one copies nothing."""
    from grand_plus_amd import _native, fit
    L = _native.lib()
    V, dim = 4097, 64
    src, dst = fr.tables(V, dim)
    s, d, dirty = _Words(src), _Words(dst), _Words(np.zeros(rm.words(V), np.uint32))
    lists = [torch.from_numpy(fr.key_lists(V)[n]).cuda() for n in ("duplicates", "strays")]
    _image, track = _track(1)

    def run():
        for k in lists:
            _native.raise_for_status(L.gp_fit_rows_mark(0, k.data_ptr(), k.numel(), V, dirty.ptr(), _stream()))
        return L.gp_fit_rows_snapshot(0, track.data_ptr(), s.ptr(), d.ptr(), V, dim, dirty.ptr(), _stream())
    _native.raise_for_status(_no_sync(run))
    bm = fr.mark(fr.mark(np.zeros(rm.words(V), np.uint32), fr.key_lists(V)["duplicates"], V), fr.key_lists(V)["strays"], V)
    want, _ = fr.snapshot(1, src, dst, bm, V)
    first = d.get().reshape(V, dim)
    assert np.array_equal(first, want) and not dirty.get().any()
    s.set(~np.asarray(src))                                                         # the table moves on; nothing is marked
    _native.raise_for_status(L.gp_fit_rows_snapshot(0, track.data_ptr(), s.ptr(), d.ptr(), V, dim, dirty.ptr(), _stream()))
    torch.cuda.synchronize()
    assert np.array_equal(d.get().reshape(V, dim), first)
    assert ctypes.sizeof(fit.GpFitTrack) == 40
