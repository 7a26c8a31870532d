"""The kernels of the atomic backward's row list (csrc/row_mark.hip) on the GPU, entry point by entry point,
against the numpy mirror of tests/row_mark_cases.py: the compaction over hand-made bitmaps, the mark over the problems of
tests/mag_cases.py against the mirror and against the key list of gp_mag_det_keys, and the zeroing of the listed rows.
Every buffer lies between guard bands that nothing may write."""
import numpy as np
import pytest
import torch

import mag_cases as mc
import row_mark_cases as rm

pytestmark = pytest.mark.gpu

G = 16                        # guard elements on either side of a buffer
NAN_BITS = 0x7FC00ABC         # the poison of `values`: a NaN with a payload, compared bit for bit


class _Ints:
    """An integer device buffer holding `a` between two guard bands of `mark`."""

    def __init__(self, a, mark):
        a = np.array(a)                                                             # a writable copy: the cases are read-only
        self.n, self.mark = a.size, mark
        self.full = torch.full((a.size + 2 * G,), mark, dtype=torch.from_numpy(a[:0]).dtype, device="cuda")
        self.full[G:G + a.size].copy_(torch.from_numpy(a))

    def ptr(self):
        return self.full.data_ptr() + G * self.full.element_size()

    def set(self, a):
        self.full[G:G + self.n].copy_(torch.from_numpy(np.array(a)))

    def get(self):
        full = self.full.cpu().numpy()
        assert (full[:G] == self.mark).all() and (full[G + self.n:] == self.mark).all(), "a guard band was written"
        return full[G:G + self.n].copy()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _compact(bm, V, cap, flag0=0, repeats=1):
    """gp_row_list_compact of the bitmap at the capacity `cap`, `repeats` times from the same bitmap: the keys with the GUARD
    elements behind them, the count, the flag and the bitmap afterwards, of the last run; the runs are bit-equal."""
    from grand_plus_amd import _native
    from grand_plus_amd import optim_rows as orows
    L = _native.lib()
    bitmap = _Ints(bm.view(np.int32), -1)                                          # the guards hold set bits: they are not the map's
    keys = _Ints(np.full(cap + rm.GUARD, rm.POISON, np.int64), rm.POISON - 1)
    count = _Ints(np.full(1, -5, np.int64), -6)
    partials = _Ints(np.full(orows.ROW_LIST_PARTIALS, -3, np.int64), -4)             # stale partials
    flag = _Ints(np.full(1, flag0, np.int32), -9)
    runs = []
    for _ in range(repeats):
        bitmap.set(bm.view(np.int32))
        keys.set(np.full(cap + rm.GUARD, rm.POISON, np.int64))
        _native.raise_for_status(L.gp_row_list_compact(0, V, bitmap.ptr(), cap, keys.ptr(), count.ptr(), partials.ptr(), flag.ptr(),
                                                       _stream()))
        torch.cuda.synchronize()
        partials.get()
        runs.append((keys.get(), int(count.get()[0]), int(flag.get()[0]), bitmap.get().view(np.uint32)))
    for r in runs[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(r, runs[0])), "two runs of the compaction differ"
    return runs[0]


def _check_compaction(bm, V, cap, label, repeats=1):
    want_keys, want_total, want_over, want_after = rm.compact(bm, V, cap)
    for flag0 in (0, 6):
        keys, total, flag, after = _compact(bm, V, cap, flag0, repeats if flag0 == 0 else 1)
        assert np.array_equal(keys, want_keys), f"{label}: the keys are not the mirror's"
        assert (keys[cap:] == rm.POISON).all() and (keys[min(want_total, cap):cap] == V).all(), label
        assert total == want_total, f"{label}: count {total}, the map holds {want_total}"
        assert flag == (flag0 | 1 if want_over else flag0), f"{label}: flag {flag} from {flag0}, overflow {want_over}"
        assert not after.any() and np.array_equal(after, want_after), f"{label}: the bitmap is not all zero afterwards"
    return want_total


@pytest.mark.parametrize("V", rm.VS + (rm.V_CHUNKS,))
def test_the_compaction_of_hand_made_bitmaps_is_the_mirror(V):
    for name, bm in rm.bitmaps(V).items():
        total = len(rm.rows_of(bm, V))
        for cap in rm.capacities(total):
            _check_compaction(bm, V, cap, f"V={V} {name} capacity {cap}", repeats=5 if name == "third" else 1)


def test_the_compaction_across_many_workgroups_and_two_tiles_a_chunk():
    """V_TILES bits: 1 024 chunks of two tiles, set bits in hundreds of them, empty chunks at the end.  Only the bitmap is
    needed, no [V, H] buffer."""
    V, bm = rm.V_TILES, rm.tiles_bitmap()
    n_words = rm.words(V)
    per = rm.chunk_words(n_words, rm.chunks(n_words))
    rows = rm.rows_of(bm, V)
    owners = np.unique((rows >> 5) // per)
    assert rm.chunks(n_words) == rm.MAX_CHUNKS and per == 2 * rm.TILE and len(owners) > 100
    assert ((((rows >> 5) % per) >= rm.TILE).any()) and rm.chunk_begin(rm.MAX_CHUNKS - 1, n_words, rm.MAX_CHUNKS) == n_words   # second tiles; empty chunks
    for cap in rm.capacities(len(rows)) + [7]:
        _check_compaction(bm, V, cap, f"V_TILES capacity {cap}", repeats=5 if cap == len(rows) else 1)


# ---- the mark
def _mark(P, col, indices, batch, V):
    """gp_row_mark_mag over the problem's tensors (col and indices possibly spoilt), into a zeroed guarded bitmap: the marked
    rows, and the bitmap's words."""
    from grand_plus_amd import _native
    bitmap = _Ints(np.zeros(rm.words(V), np.int32), 0)                             # a stray bit outside the map shows in the guards
    ip, ix, c = P.indptr.cuda(), indices.cuda(), col.reshape(-1).cuda()
    f = None if P.filled is None else P.filled.cuda()
    b = None if batch is None else batch.cuda()
    B = P.S_rows if batch is None else batch.numel()
    ptr = lambda t: None if t is None else t.data_ptr()                             # noqa: E731
    _native.raise_for_status(_native.lib().gp_row_mark_mag(0, V, ip.data_ptr(), ix.data_ptr(), P.N, c.data_ptr(), ptr(f), P.S_rows, P.K,
                                                         ptr(b), B, bitmap.ptr(), _stream()))
    torch.cuda.synchronize()
    words = bitmap.get().view(np.uint32)
    assert not (words[-1] & np.uint32(~rm.valid_mask(rm.words(V) - 1, V) & 0xFFFFFFFF)), "a bit at or above V was marked"
    return rm.rows_of(words, V)


def _det_keys(P, col, indices, batch, V):
    """The distinct in-range keys of gp_mag_det_keys with a capacity that cannot overflow."""
    from grand_plus_amd import _native
    B = P.S_rows if batch is None else batch.numel()
    cap = B * P.K * P.longest + 1
    ip, ix, c = P.indptr.cuda(), indices.cuda(), col.reshape(-1).cuda()
    f = None if P.filled is None else P.filled.cuda()
    b = None if batch is None else batch.cuda()
    base = torch.empty(B * P.K + 1, dtype=torch.int64, device="cuda")
    keys = torch.empty(cap, dtype=torch.int64, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()                             # noqa: E731
    _native.raise_for_status(_native.lib().gp_mag_det_keys(0, V, ip.data_ptr(), ix.data_ptr(), P.N, c.data_ptr(), ptr(f), P.S_rows,
                                                           P.K, ptr(b), B, cap, base.data_ptr(), keys.data_ptr(), flag.data_ptr(),
                                                           _stream()))
    k = keys.cpu().numpy()
    assert int(flag.item()) == 0
    return np.unique(k[(k >= 0) & (k < V)])


class _Spoilt:
    """A mag_cases problem with some columns and attribute ids out of range; the mirror reads the same tensors."""

    def __init__(self, P):
        self.__dict__.update(P.__dict__)
        self.col, self.indices = P.col.clone(), P.indices.clone()
        self.col[2, 0], self.col[3, 1 % P.K] = -1, P.N
        if P.K > 2:
            self.col[4, 2] = 2 ** 31 - 1
        lo = int(P.indptr[3])                                                       # node 3: in slot 0 of every row
        self.indices[lo + 1], self.indices[lo + 5], self.indices[lo + 9], self.indices[lo + 11] = -1, P.V, P.V + 31, 2 ** 31 - 1


@pytest.mark.parametrize("name", ["h7_k5_s3", "h64_k32_s2"])
@pytest.mark.parametrize("spoilt", [False, True], ids=["clean", "out-of-range"])
def test_the_marked_rows_are_the_mirrors_and_the_det_keys(name, spoilt):
    P = mc.case(name)["P"]
    assert P.filled is not None and int(P.filled[0]) == 0 and int(P.filled[1]) == P.K   # ragged: row 0 is empty, row 1 full
    if spoilt:
        P = _Spoilt(P)
    S = P.S_rows
    batches = {"none": None, "duplicated": torch.tensor([2, 0, 2, S - 1, 1, 2], dtype=torch.int32),
               "out-of-range": torch.tensor([1, -1, 3, S, 2 ** 31 - 1, -2 ** 31, 4], dtype=torch.int32),
               "empty-row-only": torch.tensor([0], dtype=torch.int32)}
    seen = set()
    for label, batch in batches.items():
        got = _mark(P, P.col, P.indices, batch, P.V)
        want = rm.marked_rows(P, None if batch is None else batch.tolist())
        assert np.array_equal(got, want), f"{name} {label}: the marked rows are not the mirror's"
        assert np.array_equal(got, _det_keys(P, P.col, P.indices, batch, P.V)), f"{name} {label}: not the distinct keys of gp_mag_det_keys"
        seen.add(len(got))
    assert 0 in seen and max(seen) > 1                                              # the empty row marks nothing


def test_no_filled_array_and_a_v_that_cuts_the_ids():
    """filled=None (every slot filled), and a V below the problem's: the ids at or above it are out of range."""
    P = mc.case("h65_k5_s16")["P"]
    assert P.filled is None
    for V in (P.V, 33, 1):
        got = _mark(P, P.col, P.indices, None, V)

        class Cut:
            pass
        cut = Cut()
        cut.__dict__.update(P.__dict__)
        cut.V = V
        want = rm.marked_rows(cut, None)
        assert np.array_equal(got, want) and (V < P.V or len(got) > 1) and (not len(got) or got.max() < V), V
        assert np.array_equal(got, _det_keys(P, P.col, P.indices, None, V))


def test_more_slots_than_the_grid_has_waves():
    """8 192 workgroups of 4 waves: with more than twice as many slots every wave goes round its loop, and the last slots
    are reached on a third trip alone."""
    P = mc.problem(1, 2, filled="full", seed=4)
    waves = rm.GRID_CAP * rm.WAVES
    B = waves + 2                                                                   # 2 * waves + 4 slots
    late = [r for r in range(P.S_rows) if len(rm.marked_rows(P, [0, r])) > len(rm.marked_rows(P, [0]))][:2]
    assert len(late) == 2
    batch = torch.zeros(B, dtype=torch.int32)
    batch[-2:] = torch.tensor(late, dtype=torch.int32)
    want = rm.marked_rows(P, [0] + late)
    assert len(want) > len(rm.marked_rows(P, [0]))                                  # the third trip's rows tell
    assert np.array_equal(_mark(P, P.col, P.indices, batch, P.V), want)


# ---- the zeroing
def _zero(V, H, keys, offset=0):
    """gp_row_list_zero over a [V, H] buffer of NaN poison that starts `offset` floats into a 16-byte aligned block: the
    buffer afterwards as uint32 bits."""
    from grand_plus_amd import _native
    full = torch.full((V * H + 2 * 64 + offset,), 0, dtype=torch.int32, device="cuda")
    full.fill_(NAN_BITS)
    at = 64 + offset
    assert full.data_ptr() % 16 == 0 and ((full.data_ptr() + 4 * at) % 16 == 0) == (offset % 4 == 0)
    k = _Ints(np.asarray(keys, np.int64), -99)
    _native.raise_for_status(_native.lib().gp_row_list_zero(0, k.ptr(), len(keys), V, H, full.data_ptr() + 4 * at, _stream()))
    torch.cuda.synchronize()
    assert np.array_equal(k.get(), np.asarray(keys, np.int64))
    bits = full.cpu().numpy().view(np.uint32)
    assert (bits[:at] == NAN_BITS).all() and (bits[at + V * H:] == NAN_BITS).all(), "the zeroing wrote outside the table"
    return bits[at:at + V * H].reshape(V, H)


@pytest.mark.parametrize("H", rm.HS)
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "unaligned"])
def test_listed_rows_become_zero_and_every_other_row_keeps_its_poison(H, offset):
    V = 37
    for rows, cap in (([0, 5, 6, 20, 36], 9), ([36], 1), ([], 4), (list(range(V)), V), ([0], 3)):
        keys = rm.list_keys(np.array(rows, np.int64), V, cap)
        bits = _zero(V, H, keys, offset)
        listed = np.zeros(V, bool)
        listed[rows] = True
        assert (bits[listed] == 0).all(), f"H={H} rows {rows}: a listed row is not +0.0f"
        assert (bits[~listed] == NAN_BITS).all(), f"H={H} rows {rows}: a row that is not listed lost its poison"


def test_more_list_positions_than_the_grid_has_waves():
    V = 2 * rm.GRID_CAP * rm.WAVES + 70
    rows = np.setdiff1d(np.arange(V), np.arange(3, V, 1001))
    bits = _zero(V, 1, rm.list_keys(rows, V, V), 0)
    listed = np.zeros(V, bool)
    listed[rows] = True
    assert (bits[listed] == 0).all() and (bits[~listed] == NAN_BITS).all()
