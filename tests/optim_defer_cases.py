"""Scenarios and the numpy mirror of the BOOKKEEPING of the embedding table's deferred exact Adam step, shared
by test_host_optim_defer.py and test_gpu_optim_defer.py.

The arithmetic has no mirror here: the GPU tests hold the deferred kernels against parent code, the dense twin
(gp_clip_adam_rows_dev in exact mode on a clone), bit for bit.  What is mirrored is csrc/optim_defer_layout.hpp: `last`, the
ring's slots and tags, the served gap and what an unserved row keeps.  `Book` replays a scenario symbolically -- for every row
the list of ring tags its updates were taken from -- with a `mistake=` switch: each of MISTAKES is one way to get the
bookkeeping wrong, and tests/test_host_optim_defer.py shows that every one of them changes what some scenario expects
(DESIGN §7q's method).

A scenario is (V, capacity, n_steps, touches, flush_after): touches[t] is the ascending array of rows the batch of step t
touches (possibly empty), flush_after the steps after which the table is flushed."""
import collections
import functools

import numpy as np

import optim_rows_cases as rc

CAPACITY = 8
V = 97
HS = (3, 8, 64, 68)
N_STEPS = 24
KINDS = ("bitmap", "det")
FLAG_BIT = 2                  # gp_optim_defer::kFlagBit
MIN_CAPACITY, MAX_CAPACITY = 4, 65536
MISTAKES = ("gap_plus_one", "gap_minus_one", "stale_slot_unchecked", "step_skips_last", "empty_writes_no_history",
            "flush_stops_early")
# the capped grids of csrc/optim_defer.hip: workgroups of the catch-up (4 list positions each per trip), of the step (4
# windows of 64 positions) and of the flush (4 waves of 64 rows)
CATCH_GRID, STEP_GRID, FLUSH_GRID, WAVES, WINDOW = 8192, 1024, 2048, 4, 64
# (max_norm, weight_decay) of the kernel tests: clipping on and off, weight decay 0 and 1e-3
SETTINGS = ((0.5, 0.0), (0.0, 1e-3), (0.5, 1e-3))
LR, BETAS, EPS = 1e-2, (0.9, 0.999), 1e-8

Scenario = collections.namedtuple("Scenario", "V capacity n_steps touches flush_after")


def _scenario(Vn, capacity, n_steps, named, flush_after, seed, lo=10, prob=0.1):
    """named: row -> the steps that touch it; every row from `lo` on is touched at random with probability `prob`."""
    rng = np.random.default_rng(seed)
    touches = {}
    for t in range(1, n_steps + 1):
        rows = {r for r, steps in named.items() if t in steps}
        if any(t in steps for steps in named.values()) or not named:
            rows |= {int(r) for r in range(lo, Vn) if rng.random() < prob}
        a = np.array(sorted(rows), dtype=np.int64)
        a.setflags(write=False)
        touches[t] = a
    return Scenario(Vn, capacity, n_steps, touches, frozenset(flush_after))


@functools.lru_cache(maxsize=None)
def main():
    """24 steps at capacity 8, flushed after steps 8, 16 and 24.  Row 0 is touched at every step but the empty one (5), row 1
    never (every flush finds it exactly `capacity` steps behind), row 2 one step after a flush (gap 1), row 3 at steps 1 and 8
    (gap capacity - 1), row 4 at step 16 alone (gap capacity: the largest served), row 5 at 2 and 10 (gap 2), row V - 1 at 7 and 23."""
    every = set(range(1, N_STEPS + 1)) - {5}
    return _scenario(V, CAPACITY, N_STEPS, {0: every, 2: {9, 17}, 3: {1, 8}, 4: {16}, 5: {2, 10}, V - 1: {7, 23}}, {8, 16, 24}, 3)


@functools.lru_cache(maxsize=None)
def wrap():
    """More than 2 x capacity steps whose replays straddle the ring's wrap: flushed after 4, 12 and 19; row 2 is touched at 10
    (replays 5 .. 9: slots 5, 6, 7, 0, 1), row 3 at 18 (13 .. 17: the same slots a turn later), row 4 at 4 and 12 (5 .. 11: seven
    slots), and the flush after 12 replays 5 .. 12, all eight slots, on every row nobody touched."""
    return _scenario(V, CAPACITY, 19, {0: set(range(1, 20)), 2: {10}, 3: {18}, 4: {4, 12}}, {4, 12, 19}, 5)


@functools.lru_cache(maxsize=None)
def single_row():
    """V = 1: touched at steps 1 and 4, flushed after 3 and 6."""
    return _scenario(1, MIN_CAPACITY, 6, {0: {1, 4}}, {3, 6}, 7)


def past_the_gap(extra):
    """Flushed after step 1; every row but row 1 is touched at step 5; rows 1 and 2 at step capacity + 1 + extra, when row 1 is
    capacity + extra steps behind: extra = 0 is the largest served gap, extra = 1 one step past it."""
    named = {r: {5} for r in range(V) if r != 1}
    named[1] = {CAPACITY + 1 + extra}
    named[2] = {5, CAPACITY + 1 + extra}
    return _scenario(V, CAPACITY, CAPACITY + 1 + extra, named, {1, CAPACITY + 1 + extra}, 11, lo=V)


def key_list(rows, Vn, kind, seed=0):
    """The rows as a list of either kind: "bitmap" -- each row once, three sentinels; "det" -- each row one to three times, a
    key below 0 in front, two sentinels (the deterministic backward's sorted keys)."""
    rows = np.asarray(rows, dtype=np.int64)
    if kind == "bitmap":
        return np.concatenate([rows, np.full(3, Vn)]).astype(np.int64)
    reps = np.random.default_rng(100 + seed).integers(1, 4, size=len(rows))
    return np.concatenate([[-1], np.repeat(rows, reps), np.full(2, Vn)]).astype(np.int64)


def gradient(keys, Vn, H, t, poisoned=False):
    """dW of step t: rc.gradient (NaN outside the touched rows), small at odd steps and large at even ones, so that with
    max_norm = 0.5 the clip coefficient is 1 at some steps and below 1 at others.  poisoned: one NaN in a touched row."""
    g = rc.gradient(keys, Vn, H, 50 + t) * np.float32(1e-3 if t % 2 else 1.0)
    if poisoned:
        g[np.flatnonzero(rc.touched(keys, Vn))[0], 0] = np.nan
    return g


class Book:
    """The bookkeeping of one deferred table, replayed symbolically.  applied[r] lists, in order, the tag of the ring entry (or,
    for a real step, the step) every update of row r was taken from: a table on the dense trajectory through step T has
    applied[r] == [1 .. T] for every row."""

    def __init__(self, Vn, capacity, tick=0, mistake=None):
        assert mistake is None or mistake in MISTAKES
        self.V, self.capacity, self.mistake = Vn, capacity, mistake
        self.last = np.full(Vn, tick, dtype=np.int64)
        self.tags = np.zeros(capacity, dtype=np.int64)
        self.flag = 0
        self.applied = [list(range(1, tick + 1)) for _ in range(Vn)]

    def _plan(self, T, last, through):
        if T >= 2 ** 31 or last < 0 or last > T:
            return "unserved"
        if last >= through:
            return "nothing"
        limit = self.capacity + {"gap_plus_one": 1, "gap_minus_one": -1}.get(self.mistake, 0)
        return "replay" if T - last <= limit else "unserved"

    def _catch_up_row(self, r, T, through):
        """True when the row is current through `through` afterwards; an unserved row keeps everything."""
        what = self._plan(T, int(self.last[r]), through)
        if what == "nothing":
            return True
        steps = range(int(self.last[r]) + 1, through + 1)
        read = [int(self.tags[s % self.capacity]) for s in steps]
        if what == "unserved" or (self.mistake != "stale_slot_unchecked" and read != list(steps)):
            self.flag |= FLAG_BIT
            return False
        self.applied[r] += read
        self.last[r] = through
        return True

    def catch_up(self, T, rows):
        if T == 0:
            return
        for r in rows:
            self._catch_up_row(int(r), T, T - 1)

    def step(self, T, rows):
        if len(rows) or self.mistake != "empty_writes_no_history":
            self.tags[T % self.capacity] = T
        for r in rows:
            r = int(r)
            if self._catch_up_row(r, T, T - 1):
                self.applied[r].append(T)
                if self.mistake != "step_skips_last":
                    self.last[r] = T

    def flush(self, T):
        for r in range(self.V):
            self._catch_up_row(r, T, T - 1 if self.mistake == "flush_stops_early" else T)

    def outcome(self):
        return self.last.tolist(), self.flag, [list(a) for a in self.applied]


def run_book(sc, mistake=None, pre_forward=True, jump=None):
    """The scenario through a Book; jump=(t, to): before step t the tick moves to `to` without a reset (a count set from
    outside), and the steps continue from there.  Returns the Book and the final tick."""
    book = Book(sc.V, sc.capacity, mistake=mistake)
    T = 0
    for t in range(1, sc.n_steps + 1):
        T = jump[1] if jump and jump[0] == t else T + 1
        if pre_forward:
            book.catch_up(T, sc.touches[t])
        book.step(T, sc.touches[t])
        if t in sc.flush_after:
            book.flush(T)
    return book, T


def gaps_seen(sc):
    """The values of T - last[r] that the catch-ups, the steps and the flushes of the scenario meet on rows that lag."""
    book, seen, T = Book(sc.V, sc.capacity), set(), 0
    for t in range(1, sc.n_steps + 1):
        T += 1
        seen |= {T - int(book.last[r]) for r in sc.touches[t]}
        book.catch_up(T, sc.touches[t])
        book.step(T, sc.touches[t])
        if t in sc.flush_after:
            seen |= {T - int(x) for x in book.last if x != T}
            book.flush(T)
    return seen
