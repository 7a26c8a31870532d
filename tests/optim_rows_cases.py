"""Key lists, shapes and the numpy mirror of the embedding table's row-list step, shared by
test_host_optim_rows.py, test_gpu_optim_rows.py and test_gpu_mag_table_step.py.

A gradient here is (dW, keys): keys is an ascending int64 list, a position is a HEAD when its key is a table row and it is
the first of its run (csrc/optim_rows_layout.hpp), a row is TOUCHED when it has a head, and dW holds NaN in every row that is
not touched -- the kernels must never read those.

`mirror_step` is the step of both modes written out in numpy, in float32 with the kernel's own operation order (or in
float64), with a `mistake=` switch: each of MISTAKES is one way to get the kernels wrong, and tests/test_host_optim_rows.py
shows that every one of them changes what some case of the grid expects (DESIGN §7q's method), so the grid can tell it.
"""
import functools
import math

import numpy as np

WINDOW = 64                   # sorted positions per wave
CHUNK = 4096                  # kRowsChunk of csrc/optim_rows.hip: table elements per unit of work in exact mode
GRID_CAP = 1024               # workgroups of one launch (the workspace's slots)
WAVES = 4                     # windows a workgroup takes at once
N_SORTED = (0, 1, 63, 64, 65, 1025)
RUNS = (1, 63, 64, 65)
MODES = ("exact", "lazy")
MISTAKES = ("pos0_not_head", "oob_key_as_row", "run_crossing_64_twice", "last_window_dropped", "lazy_decays_untouched",
            "exact_skips_untouched", "exact_reads_untouched_dW")

# (V, H) of the kernel tests: H in {1, 7, 64, 65, 257}, V in {1, 5, 64, 4097}, V * H at 4095, 4096 and 4097
SHAPES = [(1, 1), (5, 7), (64, 64), (5, 65), (5, 257), (4097, 1), (585, 7), (4096, 1), (64, 65), (1, 257)]
assert {h for _, h in SHAPES} == {1, 7, 64, 65, 257} and {v for v, _ in SHAPES} >= {1, 5, 64, 4097}
assert {4095, 4096, 4097} <= {v * h for v, h in SHAPES}
# the windows of this list exceed the grid cap twice over, so every workgroup's stride loop goes round a third time
STRIDE_SHAPE = (37, 1)
STRIDE_N = 2 * GRID_CAP * WAVES * WINDOW + 5 * WINDOW + 3


def _spread(n, V, rng):
    """n ascending keys: rows of [0, V) drawn with repeats, about a tenth of the list the sentinel V."""
    live = n - n // 10
    return np.concatenate([np.sort(rng.integers(0, V, size=live)), np.full(n - live, V)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def key_lists(V):
    """name -> ascending int64 keys for a table of V rows: every list length of N_SORTED, runs of RUNS equal keys, a run
    that starts at position 63, keys below 0 and at or above V, an all-sentinel list, rows 0 and V - 1."""
    rng = np.random.default_rng(7 * V + 1)
    out = {f"n{n}": _spread(n, V, rng) for n in N_SORTED}
    rows = sorted({0, V // 3, (2 * V) // 3, V - 1})                       # up to four distinct rows, 0 and V - 1 among them
    runs = [np.full(RUNS[i % 4], r) for i, r in enumerate(rows)]
    if len(rows) < 4:                                                     # a small table: the runs that found no row go below 0
        runs = [np.full(n, -1 - i) for i, n in reversed(list(enumerate(RUNS[len(rows):])))] + runs
    out["runs"] = np.concatenate(runs + [np.full(3, V)]).astype(np.int64)
    out["run_at_63"] = np.concatenate([np.full(63, -1), np.full(70, V - 1), np.full(2, V)]).astype(np.int64)    # crosses 64 and 128
    out["run_from_0"] = np.concatenate([np.full(130, 0), np.full(1, V)]).astype(np.int64)                      # head at 0, crosses twice
    out["out_of_range"] = np.concatenate([[-5, -5, -1], rows, [V, V, V + 3, 2 ** 40]]).astype(np.int64)
    out["all_sentinel"] = np.full(130, V, dtype=np.int64)
    out["edges"] = np.array([0, 0, V - 1], dtype=np.int64)
    out["tail_window"] = np.concatenate([np.full(64, -1), [V - 1]]).astype(np.int64)   # the only head is in the last, partial window
    for k in out.values():
        assert k.dtype == np.int64 and (np.diff(k) >= 0).all()
        k.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def stride_keys():
    V = STRIDE_SHAPE[0]
    rng = np.random.default_rng(11)
    k = np.sort(rng.integers(-1, V + 1, size=STRIDE_N)).astype(np.int64)
    k.setflags(write=False)
    assert (len(k) + WINDOW - 1) // WINDOW > 2 * GRID_CAP * WAVES
    return k


def heads(keys, V, mistake=None):
    """The head positions of the list, by brute force (or with one of MISTAKES built in)."""
    n = len(keys)
    if mistake is None and n:                                             # the same rule over whole arrays, for the long lists
        k = np.asarray(keys)
        first = np.concatenate([[True], k[1:] != k[:-1]])
        return np.flatnonzero(first & (k >= 0) & (k < V)).tolist()
    if mistake == "last_window_dropped":
        n = n // WINDOW * WINDOW
    out = []
    for i in range(n):
        k = int(keys[i])
        in_range = 0 <= k < V or mistake == "oob_key_as_row"
        first = i == 0 or int(keys[i - 1]) != k
        if mistake == "pos0_not_head" and i == 0:
            first = False
        if mistake == "run_crossing_64_twice" and i % WINDOW == 0:
            first = True
        if in_range and first:
            out.append(i)
    return out


def head_rows(keys, V, mistake=None):
    """The row every head names, one entry per head.  An out-of-range key taken as a row lands on the nearest one."""
    return [min(max(int(keys[i]), 0), V - 1) for i in heads(keys, V, mistake)]


def lower_bound(keys, row):
    """The first position whose key is >= row, by brute force."""
    for i, k in enumerate(keys):
        if int(k) >= row:
            return i
    return len(keys)


def touched(keys, V):
    """bool [V]: the rows that have a head."""
    t = np.zeros(V, dtype=bool)
    k = np.asarray(keys)
    t[k[(k >= 0) & (k < V)]] = True
    return t


def gradient(keys, V, H, seed, exact_sums=False, poison=np.nan):
    """dW float32 [V, H]: random values in the touched rows, `poison` everywhere else.  exact_sums: multiples of 2^-8 with
    |g| <= 4, so that the sum of squares is exact in float64 in any order."""
    rng = np.random.default_rng(seed)
    if exact_sums:
        g = (rng.integers(-1024, 1025, size=(V, H)) / 256.0).astype(np.float32)
    else:
        g = rng.standard_normal((V, H)).astype(np.float32)
    dW = np.full((V, H), poison, dtype=np.float32)
    t = touched(keys, V)
    dW[t] = g[t]
    return dW


def dense_gradient(dW, keys):
    """The zero-filled dense gradient that holds the same touched rows: what the dense kernel is given as the reference."""
    t = touched(keys, dW.shape[0])
    out = np.zeros_like(dW)
    out[t] = dW[t]
    return out


def state(V, H, seed):
    """(p, m, v) float32 [V, H] of a table in mid-training: every element non-zero, v positive."""
    rng = np.random.default_rng(1000 + seed)
    return ((rng.standard_normal((V, H)) * 0.1).astype(np.float32), (rng.standard_normal((V, H)) * 0.01).astype(np.float32),
            (rng.random((V, H)) * 1e-3 + 1e-6).astype(np.float32))


def corrections(lr, betas, t):
    """(step_size, rsqrt_bc2) of step t as ClipAdam forms them: in double, rounded to float32 by the call."""
    return lr / (1.0 - betas[0] ** t), 1.0 / math.sqrt(1.0 - betas[1] ** t)


def sq_norm64(dW, keys, V, mistake=None):
    """The float64 sum of squares over the rows of the heads (a row counted once per head)."""
    return float((dW[head_rows(keys, V, mistake)].astype(np.float64) ** 2).sum())


def mirror_step(mode, p, m, v, dW, keys, *, lr, betas, eps, weight_decay, clip, step_size, rsqrt_bc2, mistake=None,
                dtype=np.float32):
    """One step of the table in `mode`, in numpy: (p, m, v, norm).  dtype float32 walks the kernel's documented arithmetic
    operation by operation (the float64 norm rounded once, coef, then per element g = g coef + wd p, m = b1 m + (1 - b1) g,
    v = b2 v + (1 - b2) g g, p -= step_size (m / (sqrt(v) rsqrt_bc2 + eps))); float64 is the reference of the error bounds.
    step_size and rsqrt_bc2 are given as the kernel receives them."""
    assert mode in MODES
    V, H = p.shape
    f = dtype
    p, m, v = p.astype(f).copy(), m.astype(f).copy(), v.astype(f).copy()
    norm = f(math.sqrt(sq_norm64(dW, keys, V, mistake)))
    coef = f(1.0)
    if clip > 0:
        c = f(clip) / (norm + f(1e-6))
        coef = c if not c >= 1 else f(1.0)                                # a NaN stays a NaN
    b1, b2 = f(betas[0]), f(betas[1])
    omb1, omb2 = f(1.0 - betas[0]), f(1.0 - betas[1])

    def update(r, g):
        with np.errstate(all="ignore"):
            g = g.astype(f) * coef + f(weight_decay) * p[r]
            m[r] = b1 * m[r] + omb1 * g
            v[r] = b2 * v[r] + omb2 * g * g
            p[r] = p[r] - f(step_size) * (m[r] / (np.sqrt(v[r]) * f(rsqrt_bc2) + f(eps)))

    zero = np.zeros(H, dtype=f)
    if mode == "lazy":
        done = set()
        for r in head_rows(keys, V, mistake):                             # a row with two heads is stepped twice
            update(r, dW[r])
            done.add(r)
        if mistake == "lazy_decays_untouched":
            for r in range(V):
                if r not in done:
                    update(r, zero)
    else:
        t = touched(keys, V)
        if mistake in ("pos0_not_head", "oob_key_as_row", "last_window_dropped"):      # the touched set follows the heads
            t = np.zeros(V, dtype=bool)
            t[head_rows(keys, V, mistake)] = True
        for r in range(V):
            if t[r]:
                update(r, dW[r])
            elif mistake == "exact_reads_untouched_dW":
                update(r, dW[r])
            elif mistake != "exact_skips_untouched":
                update(r, zero)
    return p, m, v, norm


def same_bits(a, b):
    """Whether two float32 arrays hold the same bits (a NaN equals itself, +0 differs from -0)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())
