"""Shapes, inputs and exact references of the second-trip tests: tests/test_gpu_second_trip.py runs them on
the GPU, tests/test_host_second_trip.py holds them to the caps read out of the sources and shows the references exact.

Most kernels launch a capped grid and walk the rest of their work in a grid-stride loop.  Every case here is the smallest
shape that takes one such loop round twice, so the sizes are millions of elements, where the per-entry Python walks of
the other cases modules (walk_dW32, entry_order, Sampler.unlabelled) would take minutes.  The sums are therefore built to
be EXACT in float32, so that a vectorised float64 `np.bincount` cast to float32 is what the kernel must give bit for bit
whatever order it sums in (the trick of mag_det_cases.order_pin_problem and collision_cases.py):

  * weights and bag data are powers of two, and every denominator sums to exactly 1.0f, so 1 / (1 + 1e-12f) and
    1 / (1 + 1e-10f) are 1.0f;
  * eval mode: no mask and no rescale enters;
  * upstream gradients are integers with |g| <= 4;
  * destination ids are spread by a hash, so that a destination receives some hundreds of contributions (at most 2^12).

Every term is then an integer multiple of one power of two (the case's `quantum`), and every partial sum of any subset, in
any order, is below 2^24 quanta: `exact_margin` is that figure, asserted on the CPU.  No function here loops over slots,
rows or entries in Python.  Everything runs on the CPU and is computed once.
"""
import functools
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grand_plus_amd", "csrc")
f32 = np.float32
WINDOW = 64                      # sorted positions per window of gather_sum_kernel (one wave)
BLOCK = 256                      # threads of a workgroup in every kernel here but the gather (64) and MAG's rows (64 * waves)


def _find(path, pattern):
    """The integers `pattern` captures in a source file; exactly one match, or the cap moved and the cases must follow."""
    text = open(path).read()
    found = re.findall(pattern, text)
    assert len(found) == 1, f"{os.path.relpath(path, ROOT)}: {len(found)} matches of {pattern!r}"
    return [int(x) for x in (found[0] if isinstance(found[0], tuple) else (found[0],))]


@functools.lru_cache(maxsize=None)
def source_caps():
    """Every grid cap the cases pass, read out of the sources with regular expressions: name -> workgroups (or the unit
    named).  tests/test_host_second_trip.py compares them with CAPS below."""
    c = lambda name: os.path.join(CSRC, name)                                  # noqa: E731
    row_grid = _find(c("gp_common.hpp"), r"inline int row_grid\(long long n, int waves\)\s*\{[^}]*?return \(int\)\(g < (\d+) \? \(g > 0 \? g : 1\) : (\d+)\);")
    assert row_grid[0] == row_grid[1]
    assert _find(c("optim.hip"), r"constexpr int kSlots = GP_OPTIM_WORKSPACE_BYTES / (\d+);") == [8]
    assert len(re.findall(r"constexpr int kMaxGrid = kSlots;", open(c("optim.hip")).read())) == 1
    return {
        "mag_grid": _find(c("mag_stage.hpp"), r"constexpr int kGridCap = (\d+);")[0],
        "fit_grid": _find(c("fit.hip"), r"constexpr int kMaxGrid = (\d+);")[0],
        "step_grid": _find(c("step_state.hip"), r"constexpr int kMaxGrid = (\d+);")[0],
        "gather_grid": _find(c("gather_sum.hpp"), r"int gather_grid\(int64_t n_sorted\) \{ return \(int\)std::min<int64_t>\((\d+), \(n_sorted \+ 63\) / 64\); \}")[0],
        "rows_den_grid": _find(c("scatter_det.hip"), r"rows_inv_den_kernel, dim3\(std::min\(n_batch, (\d+)\)\)")[0],
        "bag_den_grid": _find(c("scatter_det.hip"), r"const int grid = \(int\)std::min<long long>\((\d+), \(n_rows \+ kBlock / 64 - 1\) / \(kBlock / 64\)\);")[0],
        "optim_chunk": _find(c("optim.hip"), r"constexpr int kChunk = (\d+);")[0],
        "optim_grid": _find(os.path.join(ROOT, "include", "grandplus.h"), r"#define GP_OPTIM_WORKSPACE_BYTES (\d+)")[0] // 8,
        "row_grid": row_grid[0],
    }


# what the cases below were sized for; a cap that moves in the sources fails the host test, and the sizes follow by hand
CAPS = {"mag_grid": 8192, "fit_grid": 4096, "step_grid": 4096, "gather_grid": 65535, "rows_den_grid": 65535,
        "bag_den_grid": 65535, "optim_chunk": 4096, "optim_grid": 1024, "row_grid": 65535}
GATHER_ONE_TRIP = CAPS["gather_grid"] * WINDOW                  # 4 194 240 sorted positions
MAG_LEN_ONE_TRIP = CAPS["mag_grid"] * BLOCK                     # 2 097 152 slots: a thread per slot
MAG_KEYS_ONE_TRIP = CAPS["mag_grid"] * (BLOCK // 64)            # 32 768 slots: a wave per slot
MAG_ROWS_ONE_TRIP = CAPS["mag_grid"]                            # batch rows: a workgroup per row
ROWS_DEN_ONE_TRIP = CAPS["rows_den_grid"]                       # batch rows: a workgroup per row
BAG_DEN_ONE_TRIP = CAPS["bag_den_grid"] * (BLOCK // 64)         # 262 140 bags: a wave per bag
STEP_ONE_TRIP = CAPS["step_grid"] * BLOCK                       # 1 048 576 mask items
FIT_ONE_TRIP = CAPS["fit_grid"] * BLOCK                         # 1 048 576 selections, or words of a snapshot
HEAD_ONE_TRIP = CAPS["row_grid"] * (BLOCK // 64)                # 262 140 rows: a wave per row
OPTIM_ONE_TRIP = CAPS["optim_grid"]                             # chunks of kChunk elements


def spread(i, salt):
    """A cheap hash of the index array i: uint64 values whose residues modulo a few thousand are close to uniform."""
    with np.errstate(over="ignore"):
        x = (np.asarray(i, dtype=np.uint64) + np.uint64(salt)) * np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(29))) * np.uint64(0xBF58476D1CE4E5B9)
    return x >> np.uint64(24)


def small_ints(i, salt):
    """Integers in [-4, 4] per index: the upstream gradients."""
    return (spread(i, salt) % np.uint64(9)).astype(np.int64) - 4


def exact_margin(dest, terms, n_dest, quantum):
    """The largest sum of |terms| over one destination, in quanta: below 2^24 every partial sum of any subset of a
    destination's terms, in any order, is an integer number of quanta that float32 holds exactly.  Also asserts that every
    term is a whole number of quanta."""
    q = np.asarray(terms, np.float64) / quantum
    assert np.array_equal(q, np.rint(q)), "a term is not a whole number of quanta"
    return float(np.bincount(dest, weights=np.abs(q), minlength=n_dest).max())


def second_trip_only(sorted_keys, n_dest, first_pos=GATHER_ONE_TRIP):
    """The destinations whose whole segment of the sorted key list lies at positions >= first_pos: bool [n_dest].  Only
    windows of the gather's second trip reach them."""
    ids = np.arange(n_dest)
    lo, hi = np.searchsorted(sorted_keys, ids, "left"), np.searchsorted(sorted_keys, ids, "right")
    return (hi > lo) & (lo >= first_pos)


# ------------------------------------------------------------------------------------------------ case 1: MAG
MAG_B, MAG_K, MAG_N, MAG_V, MAG_SLACK = 1_048_576 + 1024, 2, 4096, 8192, 1000
MAG_QUANTUM = 0.25                # g (an integer) * w' (0.5) * d (1 or 0.5)


@functools.lru_cache(maxsize=None)
def mag_case():
    """H = 1, S = 1, eval mode, K = 2: every row has val = (0.5, 0.5); node 0 has no attribute, node 1 one (d = 1.0), every
    other node two (d = 0.5, 0.5); attribute ids are a hash of the storage position modulo V = 8 192; col is a hash of the
    slot index modulo N = 4 096.  B is 1 024 past 2^20 because the bags hold at most two entries: with B * K = 2 099 200
    slots the entry total (about 4 196 900) passes the gather's 4 194 240 although some 500 slots each have none or one.

    A dict: the tensors of mag_cases.Problem (P), G float32 [B, 1], and the vectorised entry order -- slot_base, total,
    keys, sorted_keys -- with dW float32 [V, 1] = bincount(a_j, weights = (g_b * 0.5) * d_j) and `terms` (float64, per entry)."""
    import mag_cases as mc
    B, K, N, V = MAG_B, MAG_K, MAG_N, MAG_V
    n_slots = B * K
    lens = np.full(N, 2, np.int64)
    lens[0], lens[1] = 0, 1
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(indptr[-1])
    indices = (spread(np.arange(nnz), 11) % np.uint64(V)).astype(np.int32)
    data = np.full(nnz, 0.5, f32)
    data[indptr[1]] = 1.0                                                       # node 1's single entry
    col = (spread(np.arange(n_slots), 12) % np.uint64(N)).astype(np.int32)
    g = small_ints(np.arange(B), 13)
    # the vectorised entry order (b, k, t)
    slot_len = lens[col]
    slot_base = np.concatenate([[0], np.cumsum(slot_len)]).astype(np.int64)
    total = int(slot_base[-1])
    slot = np.repeat(np.arange(n_slots), slot_len)
    pos = indptr[col[slot]] + (np.arange(total) - slot_base[slot])
    keys = indices[pos].astype(np.int64)
    terms = (g[slot // K] * 0.5) * data[pos].astype(np.float64)
    dW = np.bincount(keys, weights=terms, minlength=V).astype(f32).reshape(V, 1)
    P = mc.Problem(W=torch.zeros((V, 1)), indptr=torch.from_numpy(indptr), indices=torch.from_numpy(indices),
                   data=torch.from_numpy(data), col=torch.from_numpy(col).reshape(B, K),
                   val=torch.full((B, K), 0.5, dtype=torch.float64), filled=None, K=K, N=N, V=V, H=1, S_rows=B, longest=2)
    return {"P": P, "G": torch.from_numpy(g.astype(f32)).reshape(B, 1), "slot_base": slot_base, "total": total, "keys": keys,
            "sorted_keys": np.sort(keys, kind="stable"), "terms": terms, "dW": torch.from_numpy(dW), "slot_len": slot_len,
            "kw": dict(samples=1, dropnode_rate=0.5, input_droprate=0.0, training=False, seed=1)}


# ------------------------------------------------------------------------------------------------ case 3: rows
ROWS_B, ROWS_K, ROWS_N = 65535 + 41, 64, 16384
ROWS_QUANTUM = 2.0 ** -6


@functools.lru_cache(maxsize=None)
def rows_case():
    """random_prop_rows in eval mode, F = 1, every row full with val = 2^-6 (the row denominator is 64 * 2^-6 = 1): col is a
    hash of the slot index modulo N = 16 384 (some 256 slots a node, so that about ten nodes' segments lie wholly past
    sorted position 4 194 240), G an integer per batch row.  The deterministic backward sorts all B * K slots.
    A dict with col int32 [B * K], val, filled, G float32 [B, 1], grad float32 [N, 1] = bincount(col, g_b * 2^-6)."""
    B, K, N = ROWS_B, ROWS_K, ROWS_N
    col = (spread(np.arange(B * K), 21) % np.uint64(N)).astype(np.int32)
    g = small_ints(np.arange(B), 22)
    terms = np.repeat(g, K) * ROWS_QUANTUM
    grad = np.bincount(col, weights=terms, minlength=N).astype(f32).reshape(N, 1)
    return {"col": torch.from_numpy(col), "val": torch.full((B * K,), ROWS_QUANTUM, dtype=torch.float64),
            "filled": torch.full((B,), K, dtype=torch.int32), "G": torch.from_numpy(g.astype(f32)).reshape(B, 1),
            "keys": col.astype(np.int64), "sorted_keys": np.sort(col.astype(np.int64), kind="stable"), "terms": terms,
            "grad": torch.from_numpy(grad)}


# ------------------------------------------------------------------------------------------------ case 4: bags
BAG_M, BAG_LEN, BAG_V = 262140 + 41, 16, 65536
BAG_QUANTUM = 2.0 ** -4


@functools.lru_cache(maxsize=None)
def bag_case():
    """The embedding bag in eval mode, H = 1: BAG_M bags of 16 entries with d = 2^-4 (the bag denominator is 1), attribute
    ids a hash of the storage position modulo V = 65 536 (some 64 entries an id: the 656 sorted positions past 4 194 240
    hold about ten whole segments), G an integer per bag.  A dict with the CSR (indptr int64, indices
    int32, data), G float32 [M, 1] and dW float32 [V, 1] = bincount(a_j, g_m * 2^-4)."""
    M, L, V = BAG_M, BAG_LEN, BAG_V
    indices = (spread(np.arange(M * L), 31) % np.uint64(V)).astype(np.int32)
    g = small_ints(np.arange(M), 32)
    terms = np.repeat(g, L) * BAG_QUANTUM
    dW = np.bincount(indices, weights=terms, minlength=V).astype(f32).reshape(V, 1)
    return {"indptr": torch.arange(M + 1, dtype=torch.int64) * L, "indices": torch.from_numpy(indices),
            "data": torch.full((M * L,), BAG_QUANTUM, dtype=torch.float32), "G": torch.from_numpy(g.astype(f32)).reshape(M, 1),
            "keys": indices.astype(np.int64), "sorted_keys": np.sort(indices.astype(np.int64), kind="stable"), "terms": terms,
            "dW": torch.from_numpy(dW)}


# ------------------------------------------------------------------------------------------------ case 5: the optimiser
def stride_chunks():
    """optim_cases.SETS["stride"] cut as csrc/optim.hip cuts it: (chunk_end per tensor, total chunks, and for every chunk of
    the second trip its (tensor, first element, element count))."""
    import optim_cases as oc
    sizes = [oc.numel(s) for s in oc.SETS["stride"]]
    per = [-(-n // oc.CHUNK) for n in sizes]
    ends = np.cumsum(per)
    second = []
    for c in range(OPTIM_ONE_TRIP, int(ends[-1])):                               # four chunks
        t = int(np.searchsorted(ends, c, "right"))
        start = (c - (int(ends[t - 1]) if t else 0)) * oc.CHUNK
        second.append((t, start, min(oc.CHUNK, sizes[t] - start)))
    return ends.tolist(), int(ends[-1]), second


# ------------------------------------------------------------------------------------------------ case 6: the masks
MASK_S, MASK_K, MASK_B, MASK_ROWS, MASK_WIDTH = 16, 64, 1025, 1040, 33
MASK_ROW_ITEMS = MASK_S * MASK_B * MASK_K                       # 1 049 600: the segment boundary lies on the second trip
MASK_ITEMS = MASK_ROW_ITEMS + MASK_S * MASK_B * MASK_WIDTH


@functools.lru_cache(maxsize=None)
def mask_case():
    """(filled int32 [MASK_ROWS] ragged in 0 .. K, batch_rows int32 [MASK_B]: distinct resident rows in a shuffled order)."""
    rng = np.random.default_rng(61)
    filled = rng.integers(0, MASK_K + 1, MASK_ROWS).astype(np.int32)
    filled[:3] = (0, MASK_K, 1)
    rows = rng.permutation(MASK_ROWS)[:MASK_B].astype(np.int32)
    return torch.from_numpy(filled), torch.from_numpy(rows)


# ------------------------------------------------------------------------------------------------ cases 7 and 8: the fit loop
SELECT_TRAIN, SELECT_UNLABEL = 3, FIT_ONE_TRIP + 300
SELECT_TOTAL = SELECT_TRAIN + SELECT_UNLABEL
# selection indices whose unlabelled entry is held to perm_index: the first 64, the 128 round index 1 048 576, the last 64
SELECT_PROBES = np.concatenate([np.arange(SELECT_TRAIN, SELECT_TRAIN + 64), np.arange(FIT_ONE_TRIP - 64, FIT_ONE_TRIP + 64),
                                np.arange(SELECT_TOTAL - 64, SELECT_TOTAL)])
SNAPSHOT_WORDS = (5, FIT_ONE_TRIP + 4097, 7)                    # the boundary into the third tensor lies on the second trip


# ------------------------------------------------------------------------------------------------ case 9: the head
HEAD_N = HEAD_ONE_TRIP + 37
HEAD_C = (3, 65)
HEAD_IGNORE = -100


@functools.lru_cache(maxsize=None)
def head_case(C):
    """(z float32 [HEAD_N, C], y int64 [HEAD_N], y_valid): random logits of a few units; labels in [0, C) but every 97th
    ignored and every 101st out of range (C + 5 and -1 in turn), some of each among the last 37 rows.  y_valid is y with
    the out-of-range labels ignored too: what torch's nll_loss can be given."""
    g = torch.Generator().manual_seed(7000 + C)
    z = torch.randn((HEAD_N, C), generator=g) * 3.0
    y = torch.randint(0, C, (HEAD_N,), generator=g)
    i = torch.arange(HEAD_N)
    y[i % 97 == 0] = HEAD_IGNORE
    y[i % 202 == 1] = C + 5
    y[i % 202 == 102] = -1
    y[HEAD_N - 30], y[HEAD_N - 20], y[HEAD_N - 10] = HEAD_IGNORE, C + 5, -1
    y_valid = torch.where((y >= 0) & (y < C), y, torch.full_like(y, HEAD_IGNORE))
    return z, y, y_valid
