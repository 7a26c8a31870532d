"""Cases, the order contract as a numpy float32 walk, and the deliberate mistakes of the chunked deterministic segment sums
(csrc/gather_chunk_abi.hpp).  tests/test_host_gather_chunk.py audits the cases on the CPU,
tests/test_gpu_gather_chunk.py runs them on the GPU.

A case is a key list placed by hand: `segs` are the segment lengths of destinations 0, 1, 2 ... in sorted order, `dead`
entries carry an id outside the table (the sentinel tail).  The entries are shuffled, so that the stable sort has work to
do; every entry is a bag of its own with weight 1.0, so that 1 / (1 + 1e-10f) is exactly 1.0f and what sorted position q
contributes is the upstream gradient row of its entry, bit for bit (test_gpu_deterministic_backward.py's construction).
Everything here runs on the CPU and is computed once.
"""
import functools

import numpy as np

f32 = np.float32
WINDOW = 64


# ------------------------------------------------------------------------------------------------ the contract
def _sum(rows, width):
    """The left-to-right float32 sum of rows [n, width], from 0.0f."""
    acc = np.zeros(width, f32)
    for r in rows:
        acc = (acc + r).astype(f32)
    return acc


def _segments(sorted_keys, n_dest):
    """(dest, q0, n) of every run of equal keys in [0, n_dest)."""
    keys = np.asarray(sorted_keys, np.int64)
    out, q = [], 0
    while q < len(keys):
        e = q
        while e < len(keys) and keys[e] == keys[q]:
            e += 1
        if 0 <= keys[q] < n_dest:
            out.append((int(keys[q]), q, e - q))
        q = e
    return out


def _cut(sorted_keys, terms, n_dest, bounds, reverse=False):
    """dst [n_dest, W]: per segment, `bounds(q0, n)` gives the chunk boundaries 0 = b_0 < b_1 < ... <= n (offsets into the
    segment); each chunk is summed left to right from 0.0f, and the partials are summed from 0.0f in chunk order (or in
    reverse).  Offsets past the last boundary are left out."""
    terms = np.asarray(terms, f32)
    W = terms.shape[1]
    dst = np.zeros((n_dest, W), f32)
    for dest, q0, n in _segments(sorted_keys, n_dest):
        b = bounds(q0, n)
        partials = [_sum(terms[q0 + lo:q0 + hi], W) for lo, hi in zip(b[:-1], b[1:])]
        dst[dest] = _sum(partials[::-1] if reverse else partials, W)
    return dst


def _from_start(C):
    return lambda q0, n: list(range(0, n, C)) + [n]


def chunked_sum(sorted_keys, terms, n_dest, C):
    """The order contract of gather_chunk_abi.hpp: terms [n_sorted, W] float32, what each sorted position contributes
    (zeros for a position that contributes nothing); float32 [n_dest, W]."""
    return _cut(sorted_keys, terms, n_dest, _from_start(C))


def left_to_right(sorted_keys, terms, n_dest):
    """The unchunked contract: one chunk per segment."""
    return _cut(sorted_keys, terms, n_dest, lambda q0, n: [0, n])


# ------------------------------------------------------------------------------------------------ deliberate mistakes
def _window_aligned(C):
    def bounds(q0, n):                                  # chunks counted from the start of the 64-position window q0 lies in
        first = C - q0 % WINDOW
        return [0] + list(range(first, n, C)) + [n] if first < n else [0, n]
    return bounds


def _drop_last_short(C):
    def bounds(q0, n):
        return list(range(0, n, C)) + ([n] if n % C == 0 or n < C else [])
    return bounds


# name -> (what the mistaken kernel would compute, which segments (q0, n) tell it from the contract by construction)
MISTAKES = {
    "plain left to right": (lambda k, t, d, C: left_to_right(k, t, d), lambda q0, n, C: n > C + 1),
    "chunks aligned to the window": (lambda k, t, d, C: _cut(k, t, d, _window_aligned(C)), lambda q0, n, C: n > C and q0 % WINDOW != 0),
    "partials folded in reverse": (lambda k, t, d, C: _cut(k, t, d, _from_start(C), reverse=True), lambda q0, n, C: n > 2 * C),
    "chunk C/2": (lambda k, t, d, C: _cut(k, t, d, _from_start(C // 2)), lambda q0, n, C: n > C // 2),
    "chunk 2C": (lambda k, t, d, C: _cut(k, t, d, _from_start(2 * C)), lambda q0, n, C: n > C + 1),
    "last short chunk dropped": (lambda k, t, d, C: _cut(k, t, d, _drop_last_short(C)), lambda q0, n, C: n > C and n % C != 0),
}
# A fold of two partials is the same in both directions (fp32 addition commutes); a segment of C + 1 entries is
# partial_0 + x_C under the contract, which is the plain walk (and the walk of chunk 2C); a segment that starts at a
# window's first position has the window's chunks.


# ------------------------------------------------------------------------------------------------ the cases
def _case(name, C, segs, dead=0, H=(1, 64, 65, 257), target=None):
    return {"name": name, "C": C, "segs": list(segs), "dead": dead, "H": tuple(H), "target": target}


def _lone(C, n, start):
    """One destination of n entries that starts at sorted position `start`, behind fillers of at most 64 entries each."""
    fill = [] if start == 0 else [start] if start <= 64 else [64, start - 64]
    return fill + [n], len(fill)


def _cases():
    out = []
    for n in (63, 64, 65, 127, 128, 129, 4097):
        for start in (0, 1, 63, 64):
            segs, t = _lone(64, n, start)
            # 4 097 entries (65 chunks, a walk of many windows) at H = 1 and 65, and with the second kCols pass (257) at start 63
            H = (1, 64, 65, 257) if n < 4097 else (1, 65, 257) if start == 63 else (1, 65)
            out.append(_case(f"c64_n{n}_at{start}", 64, segs, dead=3, target=t, H=H))
    for n in (256, 257, 513):
        segs, t = _lone(256, n, 1)
        out.append(_case(f"c256_n{n}_at1", 256, segs, dead=3, target=t, H=(65, 257) if n == 513 else (65,)))
    # A (129: a last chunk of one entry) then long B (130) then a short one; A's last chunk at q % 64 == 10, where B's
    # chunk 0 starts in the same span (both scratch rows of that span in use), and at q % 64 == 63, a window's last lane
    for pad in (10, 63):
        out.append(_case(f"adjacent_at{pad}", 64, [pad, 129, 130, 5], dead=7, target=1, H=(1, 65)))
    out.append(_case("long_ends_the_list", 64, [5, 200], dead=0, target=1, H=(65,)))
    out.append(_case("long_into_the_tail", 64, [5, 200], dead=40, target=1, H=(65,)))
    out.append(_case("all_sentinel", 64, [], dead=130, H=(65,)))
    return out


CASES = {c["name"]: c for c in _cases()}


@functools.lru_cache(maxsize=None)
def entries(name, H):
    """The case as entries: dest int64 [n] (-1: an id outside the table), G float32 [n, H] (the upstream gradient row of
    every entry, magnitudes spread over seven decades so that every grouping of a sum rounds differently), and the sorted
    view: order (stable), sorted_keys (the sentinel n_dest in the tail), terms = G[order] with zeros in the tail."""
    c = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)) * 1000 + H)
    n_dest = len(c["segs"]) + 2                         # two destinations that nothing names
    dest = np.concatenate([np.full(n, k, np.int64) for k, n in enumerate(c["segs"])] + [np.full(c["dead"], -1, np.int64)])
    dest = dest[rng.permutation(len(dest))]
    G = (rng.standard_normal((len(dest), H)) * 10.0 ** rng.integers(-3, 4, (len(dest), 1))).astype(f32)
    keys = np.where(dest >= 0, dest, n_dest)
    order = np.argsort(keys, kind="stable")
    terms = G[order].copy()
    terms[keys[order] == n_dest] = 0
    return {"dest": dest, "G": G, "n_dest": n_dest, "order": order, "sorted_keys": keys[order], "terms": terms, "C": c["C"]}


@functools.lru_cache(maxsize=None)
def expected(name, H):
    e = entries(name, H)
    return chunked_sum(e["sorted_keys"], e["terms"], e["n_dest"], e["C"])


def pins(name):
    """The mistakes this case tells from the contract by construction: those whose rule holds for one of its segments."""
    c = CASES[name]
    starts = np.concatenate([[0], np.cumsum(c["segs"])])
    return [m for m, (_, rule) in MISTAKES.items() if any(rule(int(q0), n, c["C"]) for q0, n in zip(starts, c["segs"]))]


# ------------------------------------------------------------------------------------------------ the kernels' mapping
def seg_start_of(keys, base, key):
    """gather_chunk_layout.hpp's seg_start_of, line by line."""
    hi, step = base - 1, 1
    while hi - step >= 0 and keys[hi - step] >= key:
        hi -= step
        step <<= 1
    lo = hi - step + 1 if hi - step >= 0 else 0
    while lo < hi:
        mid = lo + (hi - lo) // 2
        if keys[mid] >= key:
            hi = mid
        else:
            lo = mid + 1
    return lo


def mapping_model(sorted_keys, terms, n_dest, C):
    """What the two kernels of gather_chunk.hpp do, window by window, in numpy: the chunk heads of every window of 64
    positions (a first position of a run, or a position a multiple of C past its run's start, the start of the run that
    enters the window found by seg_start_of), a walk of at most C positions per head into dst or into scratch row
    2 * (q // C) + (chunk == 0), then the fold.  The scratch starts as NaN and every row is written at most once.
    Returns (dst, rows of the scratch that were written)."""
    keys = np.asarray(sorted_keys, np.int64)
    terms = np.asarray(terms, f32)
    n, W = len(keys), terms.shape[1]
    dst = np.zeros((n_dest, W), f32)
    scratch = np.full((2 * ((n + C - 1) // C), W), np.nan, f32)
    written = []
    valid = (keys >= 0) & (keys < n_dest)
    first = valid & np.concatenate([[True], keys[1:] != keys[:-1]])
    is_long = lambda q: q + C < n and keys[q + C] == keys[q]                      # noqa: E731
    for base in range(0, n, WINDOW):
        entered = seg_start_of(keys, base, keys[base]) if valid[base] and not first[base] else base
        seg_start = entered
        for q in range(base, min(base + WINDOW, n)):
            if first[q]:
                seg_start = q
            if not valid[q] or (q - seg_start) % C:
                continue
            p = (q - seg_start) // C
            end = q
            while end < n and end - q < C and keys[end] == keys[q]:
                end += 1
            part = _sum(terms[q:end], W)
            if p == 0 and not is_long(q):
                dst[keys[q]] = part
            else:
                slot = 2 * (q // C) + (1 if p == 0 else 0)
                assert slot not in written, f"scratch row {slot} written twice"
                written.append(slot)
                scratch[slot] = part
    for q0 in np.flatnonzero(first):
        if not is_long(q0):
            continue
        parts, p = [], 0
        while q0 + p * C < n and keys[q0 + p * C] == keys[q0]:
            parts.append(scratch[2 * ((q0 + p * C) // C) + (1 if p == 0 else 0)])
            p += 1
        dst[keys[q0]] = _sum(parts, W)
    return dst, sorted(written)
