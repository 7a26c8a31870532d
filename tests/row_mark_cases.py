"""Bitmaps, shapes and the numpy mirror of the atomic backward's row list, shared by test_host_row_mark.py,
test_gpu_row_mark.py and test_gpu_mag_atomic_rows.py.

A bitmap is uint32 [words(V)]: row r is bit r & 31 of word r >> 5 (csrc/row_mark_layout.hpp).  `compact` is the compaction
written out in numpy, chunk by chunk as the two launches of csrc/row_mark.hip cut it, and `marked_rows` the mark kernel's
enumeration of a batch's slots, each with a `mistake=` switch: every one of MISTAKES is one way to get the kernels wrong,
and tests/test_host_row_mark.py shows that each changes what some case of the grid expects (DESIGN §7q's method).

The key buffer of a case is `capacity` keys followed by GUARD more, which nothing may write: a mistake that writes past
the capacity shows there.
"""
import functools

import numpy as np

TILE = 256                    # kTile of csrc/row_mark_layout.hpp: words a workgroup scans at a time
MAX_CHUNKS = 1024             # kMaxChunks: workgroups of the compaction
GRID_CAP = 8192               # kGridCap of csrc/mag_stage.hpp: workgroups of the mark and zero kernels
WAVES = 4                     # waves of such a workgroup: slots or list positions taken at once
GUARD = 8
POISON = -7                   # what a key buffer holds before the call
VS = (1, 31, 32, 33, 63, 64, 65, 4097)
V_CHUNKS = 3 * TILE * 32 + 5                                   # four chunks of one tile, the last a single partial word
# more tiles than chunks: every workgroup owns two tiles (the last ones fewer), and set bits lie in many of them
V_TILES = (MAX_CHUNKS * TILE + 300) * 32 + 17
HS = (1, 7, 64, 65, 257)
MISTAKES = ("bit_order_reversed", "last_partial_word_dropped", "bit_above_v_emitted", "tail_not_filled",
            "offset_from_wrong_partial", "bitmap_not_cleared", "truncated_per_chunk", "dropped_slot_not_marked")


def words(V):
    return (V + 31) >> 5


def chunks(n_words):
    return min(max((n_words + TILE - 1) // TILE, 1), MAX_CHUNKS)


def chunk_words(n_words, n_chunks):
    per = (n_words + n_chunks - 1) // n_chunks
    return (per + TILE - 1) // TILE * TILE


def chunk_begin(c, n_words, n_chunks):
    return min(c * chunk_words(n_words, n_chunks), n_words)


def valid_mask(w, V):
    left = V - 32 * w
    return 0xFFFFFFFF if left >= 32 else 0 if left <= 0 else (1 << left) - 1


def bitmap_of(V, rows, stray=False):
    """The bitmap of V bits with `rows` set.  stray: the bits of the last word at or above V are set too -- the kernels
    never set them, and the compaction must not list them whatever the word holds."""
    bm = np.zeros(words(V), dtype=np.uint32)
    rows = np.asarray(rows, dtype=np.int64)
    assert ((rows >= 0) & (rows < V)).all()
    np.bitwise_or.at(bm, rows >> 5, np.uint32(1) << (rows & 31).astype(np.uint32))
    if stray:
        bm[-1] |= np.uint32(~valid_mask(words(V) - 1, V) & 0xFFFFFFFF)
    return bm


def rows_of(bitmap, V):
    """The set rows below V, ascending, by brute force over the bits."""
    return np.flatnonzero(np.unpackbits(np.ascontiguousarray(bitmap, dtype=np.uint32).view(np.uint8), bitorder="little")[:V]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def bitmaps(V):
    """name -> (uint32 bitmap, read-only) for a table of V rows: empty, full, the single bits at row 0 and at row V - 1,
    both ends, a random third of the rows, and the full and the empty map with the stray bits above V set."""
    rng = np.random.default_rng(13 * V + 5)
    third = np.flatnonzero(rng.random(V) < 1.0 / 3.0)
    out = {"empty": bitmap_of(V, []), "full": bitmap_of(V, np.arange(V)), "row0": bitmap_of(V, [0]), "last": bitmap_of(V, [V - 1]),
           "ends": bitmap_of(V, [0, V - 1]), "third": bitmap_of(V, third), "full_stray": bitmap_of(V, np.arange(V), stray=True),
           "empty_stray": bitmap_of(V, [], stray=True)}
    for b in out.values():
        b.setflags(write=False)
    return out


def capacities(total):
    """The capacities a bitmap with `total` rows is compacted at: the total, one below and one above (at least 1)."""
    return sorted({max(1, total - 1), max(1, total), total + 1})


@functools.lru_cache(maxsize=None)
def tiles_bitmap():
    """The bitmap of V_TILES bits: a bit every 4 099 rows (a prime: every bit position of a word occurs), the first and
    the last row."""
    rows = np.unique(np.concatenate([np.arange(0, V_TILES, 4099), [0, V_TILES - 1]]))
    bm = bitmap_of(V_TILES, rows)
    bm.setflags(write=False)
    return bm


def compact(bitmap, V, capacity, mistake=None, slow=False):
    """(keys int64 [capacity + GUARD], count, overflowed, the bitmap afterwards) of gp_row_list_compact.  Without a mistake
    the answer comes from the bits by brute force; slow=True or a mistake walks the chunks as the kernels do."""
    bm = np.ascontiguousarray(bitmap, dtype=np.uint32)
    assert bm.shape == (words(V),) and capacity >= 1
    keys = np.full(capacity + GUARD, POISON, dtype=np.int64)
    if mistake is None and not slow:
        rows = rows_of(bm, V)
        n = min(len(rows), capacity)
        keys[:n] = rows[:n]
        keys[n:capacity] = V
        return keys, len(rows), len(rows) > capacity, np.zeros_like(bm)
    n_words = words(V)
    n_chunks = chunks(n_words)
    seen = V // 32 if mistake == "last_partial_word_dropped" else n_words

    def live(w):
        word = int(bm[w])
        return word if mistake == "bit_above_v_emitted" else word & valid_mask(w, V)

    span = [(min(chunk_begin(c, n_words, n_chunks), seen), min(chunk_begin(c + 1, n_words, n_chunks), seen)) for c in range(n_chunks)]
    partials = [sum(bin(live(w)).count("1") for w in range(lo, hi)) for lo, hi in span]
    total = sum(partials)
    for c, (lo, hi) in enumerate(span):
        pos = sum(partials[:c - 1] if mistake == "offset_from_wrong_partial" and c >= 1 else partials[:c])
        local = 0
        for w in range(lo, hi):
            word = live(w)
            bits = [b for b in range(32) if (word >> b) & 1]
            if mistake == "bit_order_reversed":
                bits.reverse()
            for b in bits:
                fits = local < capacity if mistake == "truncated_per_chunk" else pos < capacity
                if fits and pos < len(keys):
                    keys[pos] = 32 * w + b
                pos += 1
                local += 1
    if mistake != "tail_not_filled":
        keys[min(total, capacity):capacity] = V
    after = bm.copy() if mistake == "bitmap_not_cleared" else np.zeros_like(bm)
    return keys, total, total > capacity, after


def marked_rows(P, batch, kept=None, mistake=None):
    """The rows gp_row_mark_mag marks for a batch of the problem P (tests/mag_cases.py; batch: an int sequence or None for
    every row): every in-range attribute id of the bag of every slot that exists -- a batch row in [0, S_rows), k below
    min(filled, K), a column in [0, N) -- whether or not DropNode kept the slot (kept: bool per slot e = b * K + k, used by
    the mistake alone).  Ascending int64."""
    col, K = P.col.reshape(-1).numpy(), P.K
    indptr, indices = P.indptr.numpy(), P.indices.numpy()
    filled = None if P.filled is None else P.filled.numpy()
    rows = range(P.S_rows) if batch is None else [int(r) for r in batch]
    out = set()
    for b, r in enumerate(rows):
        if not 0 <= r < P.S_rows:
            continue
        n = K if filled is None else min(int(filled[r]), K)
        for k in range(n):
            node = int(col[r * K + k])
            if not 0 <= node < P.N:
                continue
            if mistake == "dropped_slot_not_marked" and kept is not None and not kept[b * K + k]:
                continue
            out.update(int(a) for a in indices[indptr[node]:indptr[node + 1]] if 0 <= int(a) < P.V)
    return np.array(sorted(out), dtype=np.int64)


def list_keys(rows, V, capacity):
    """The list of `capacity` keys that names `rows` (ascending, distinct): the rows, then the sentinel V."""
    keys = np.full(capacity, V, dtype=np.int64)
    n = min(len(rows), capacity)
    keys[:n] = np.asarray(rows[:n], dtype=np.int64)
    return keys
