"""Shapes, key lists, bitmaps and the numpy mirror of the dirty-row snapshot (csrc/fit_rows.hip), shared by
test_host_fit_rows.py and test_gpu_fit_rows.py.

The dirty bitmap is the row list's (tests/row_mark_cases.py: uint32 [words(V)], row r is bit r & 31 of word r >> 5).
`mark` is gp_fit_rows_mark and `snapshot` gp_fit_rows_snapshot written out in numpy over 32-bit words: the kernels move
bits, so the tables are uint32 and hold NaNs with payloads and negative zeros.
"""
import functools

import numpy as np

import row_mark_cases as rm

GRID_CAP = 2048               # kMaxGrid of csrc/fit_rows.hip: workgroups of either kernel
WAVES = 4                     # kWaves of csrc/fit_rows_layout.hpp: waves of a workgroup, a word each
VS = (1, 31, 32, 33, 4097)
DIMS = (1, 7, 64, 65, 257)
V_PAST_CAP = (GRID_CAP * WAVES + 5) * 32 + 3                   # five words and a partial one past one trip of the full grid
V_TWO_TRIPS = 2 * GRID_CAP * WAVES * 32                        # with dim = 1: every wave goes round its loop exactly twice
FIRST_TRIP_ROWS = GRID_CAP * WAVES * 32                        # the rows whose words a wave owns on its first trip
NAN_BITS, NEG_ZERO = 0x7FC00ABC, 0x80000000


def key_lists(V):
    """name -> int64 key list for a table of V rows: duplicates (the sorted keys of the deterministic backward), each row
    once with the sentinel V in the tail (the compacted list), the empty list, sentinels alone, and a list with a negative
    key and a key above V before the tail."""
    rng = np.random.default_rng(7 * V + 1)
    some = np.sort(rng.integers(0, V, max(3, V // 3)))
    once = np.unique(some)
    return {"duplicates": np.concatenate([some, some[:2]]).astype(np.int64),                    # the last two: out of order too
            "tail": np.concatenate([once, np.full(5, V)]).astype(np.int64),
            "empty": np.zeros(0, np.int64),
            "sentinels": np.full(4, V, np.int64),
            "strays": np.concatenate([[-1, -2 ** 40], once[:1], [V + 7, 2 ** 40], once[1:], [V - 1], np.full(3, V)]).astype(np.int64)}


def mark(dirty, keys, V):
    """The bitmap after gp_fit_rows_mark: every key in [0, V) sets its bit, bits already set stay."""
    keys = np.asarray(keys, np.int64)
    rows = keys[(keys >= 0) & (keys < V)]
    return np.ascontiguousarray(dirty, dtype=np.uint32) | rm.bitmap_of(V, rows)


def foreign(V):
    """A bitmap with bits already set before the mark: every fifth row and the last."""
    return rm.bitmap_of(V, np.unique(np.concatenate([np.arange(0, V, 5), [V - 1]])))


@functools.lru_cache(maxsize=None)
def bitmaps(V):
    """name -> (uint32 bitmap, read-only): empty, full, the single bits at rows 0, 31, 32 and V - 1 (those below V), a random
    third, and maps whose last word also holds bits at or above V."""
    out = {"empty": rm.bitmap_of(V, []), "full": rm.bitmap_of(V, np.arange(V)), "third": rm.bitmaps(V)["third"].copy(),
           "full_stray": rm.bitmap_of(V, np.arange(V), stray=True), "stray_alone": rm.bitmap_of(V, [], stray=True)}
    for r in (0, 31, 32, V - 1):
        if 0 <= r < V:
            out[f"row{r}"] = rm.bitmap_of(V, [r])
    for b in out.values():
        b.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def tables(V, dim):
    """(src, dst) uint32 [V, dim]: the source random bits with NaNs (payloads kept) and negative zeros sprinkled in, the
    destination a distinct pattern that tells its own position."""
    rng = np.random.default_rng(1000 * dim + V)
    src = rng.integers(0, 2 ** 32, (V, dim), dtype=np.uint64).astype(np.uint32)
    flat = src.reshape(-1)
    flat[::3] = NAN_BITS
    flat[1::7] = NEG_ZERO
    flat[2::11] = 0xFFFFFFFF                                                        # a negative NaN, every payload bit set
    dst = (np.arange(V * dim, dtype=np.uint64) % 0x00FFFFFF).astype(np.uint32).reshape(V, dim) | np.uint32(0xD5000000)
    assert not (src == dst).any()
    src.setflags(write=False)
    dst.setflags(write=False)
    return src, dst


def snapshot(copy_now, src, dst, dirty, V):
    """(dst, dirty) after gp_fit_rows_snapshot."""
    dirty = np.ascontiguousarray(dirty, dtype=np.uint32)
    if not copy_now:
        return dst.copy(), dirty.copy()
    out = dst.copy()
    rows = rm.rows_of(dirty, V)
    out[rows] = src[rows]
    return out, np.zeros_like(dirty)
