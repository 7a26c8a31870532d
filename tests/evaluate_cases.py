"""Inputs, references and bounds shared by tests/test_gpu_evaluate.py, tests/test_gpu_evaluate_edges.py and the audit of
tests/test_host_mutants.py.

The references are torch's own `F.nll_loss(F.log_softmax(z))` in float64 on the CPU for the head, and for the end-to-end
checks the float64 chain of the oracles: `oracle.random_prop_ref` (or `oracle.predict_ref.propagate_ref`) ->
`oracle.mlp_ref.RefMLP` -> log-softmax -> argmax.  Everything here runs on the CPU and is computed once per case."""
import functools

import numpy as np
import torch
import torch.nn.functional as Fn

from augment_cases import rows_to_coo
from oracle.mlp_ref import RefMLP
from oracle.objective_ref import grand_loss_ref
from oracle.predict_ref import propagate_ref
from oracle.random_prop_ref import random_prop_ref

HEAD_C = (1, 3, 7, 64, 65, 349)
HEAD_N = (1, 63, 64, 65, 4097)
WRONG, CORRECT, IGNORED, BAD = 0, 1, 2, 3

# Cora's shape (run_cora.sh): F, hidden, classes, layers; K of the rows; the two models of the end-to-end tests as
# (use_bn, node_norm).  FIRST_SCALE and LAST_SCALE multiply the first and last layer's weights so that the predictions
# spread over the classes and float64 top-2 logit gaps are far above the fp32 error bound for all but a few rows
# (asserted before every prediction comparison: at most LEFT_OUT of them).
F_IN, HIDDEN, CLASSES, LAYERS, K_ROWS = 1433, 64, 7, 2, 32
MODELS = {"plain": (False, False), "bn_norm": (True, True)}
FIRST_SCALE, LAST_SCALE = 8.0, 4.0
LEFT_OUT = 0.01


@functools.lru_cache(maxsize=None)
def head_case(n, C):
    """(z float32 [n, C], y int64 [n], ref64): random logits of a few units, labels in [0, C), torch's float64 loss."""
    g = torch.Generator().manual_seed(1000 * C + n)
    z = torch.randn((n, C), generator=g) * 3.0
    y = torch.randint(0, C, (n,), generator=g)
    return z, y, float(nll64(z, y))


def nll64(z, y, ignore_index=-100):
    return Fn.nll_loss(Fn.log_softmax(z.double().cpu(), dim=-1), y.cpu(), ignore_index=ignore_index)


def nll32_on(z, y, ignore_index=-100):
    """The same torch call in float32 where z lives (the GPU in the tests): what the project's rule measures ours by."""
    return float(Fn.nll_loss(Fn.log_softmax(z, dim=-1), y, ignore_index=ignore_index))


def assert_loss(ours, torch32, ref64, what):
    """§7g's rule: |ours - ref64| <= 4 |torch32 - ref64| + 2^-23 |ref64|.  Prints the ratio ours / torch32 first."""
    e_ours, e_t = abs(ours - ref64), abs(torch32 - ref64)
    print(f"[evaluate] {what}: |ours-ref64| {e_ours:.3e}  |torch32-ref64| {e_t:.3e}  ratio {e_ours / e_t if e_t else float('nan'):.3g}")
    assert e_ours <= 4.0 * e_t + 2.0 ** -23 * abs(ref64), (what, ours, torch32, ref64)


def ties_case():
    """(z [8, 349], y): ties across lanes and passes, NaNs, a row of -inf and one +inf; labels ignored but for four rows."""
    C = 349
    z = torch.randn((8, C), generator=torch.Generator().manual_seed(5))
    z[0, [0, 63, 64]] = 9.0                                  # lanes 0 / 63 and the second pass of lane 0
    z[1, [63, 64]] = 9.0
    z[2, [64, 128, 320]] = 9.0                               # the same lane, three passes
    z[3, [348, 100]] = 9.0
    z[4, 70] = float("nan"); z[4, 5] = float("nan")          # the first NaN wins
    z[5, 64] = float("nan"); z[5, 3] = 50.0                  # a NaN beats every number
    z[6, :] = float("-inf")                                  # all equal: index 0
    z[7, 10] = float("inf")
    y = torch.full((8,), -100, dtype=torch.int64)            # ignored: the loss of a NaN row is not the subject here
    y[:4] = torch.tensor([0, 63, 64, 100])
    return z, y


def ignored_case():
    """(z [300, 7], clean labels, labels with ignored and bad entries, rows, label_rows, ignored positions, bad positions)."""
    n, C = 300, 7
    z, y, _ = head_case(4097, C)
    z, y = z[:n].clone(), y[:n].clone()
    y2 = y.clone()
    y2[[3, 77]] = -100                                       # ignore_index
    y2[[5, 100]] = torch.tensor([C, -1])                     # labels outside [0, C)
    y2[200] = 2 ** 40
    rows, lrows = torch.arange(n), torch.arange(n)
    rows[[9, 10]] = torch.tensor([n, -1])                    # a logits row outside the array
    lrows[[11, 12]] = torch.tensor([n, -(2 ** 50)])          # a label index outside the array
    return z, y, y2, rows, lrows, [3, 77], [5, 100, 200, 9, 10, 11, 12]


# ---- the head written out in float64, and one deliberate mistake (tests/test_host_mutants.py)
BOOKKEEPING = ("acc_over_valid", "loss_over_rows", "tie_last_index", "nan_not_max", "ignored_in_loss")
# arithmetic mistakes of the head, judged on EDGE_DRAWN row by row against row_bound64, and of the reduce (reduce64)
HEAD_ARITHMETIC = ("no_max_subtraction", "lse_first_pass_only", "lse_tail_dropped", "max_first_pass_only", "gather_y_mod_64",
                   "nll_of_pred", "lse_sign")
REDUCE_MUTANTS = ("reduce_in_float32", "reduce_last_slice_dropped")
MUTANTS = BOOKKEEPING + HEAD_ARITHMETIC + REDUCE_MUTANTS
# A mistake that no drawn case can tell from the correct head would be named here with its reason, as
# objective_cases.INDISTINGUISHABLE does; every mistake of MUTANTS is seen.
INDISTINGUISHABLE = ()
WRITTEN_OUT = "written_out"                                  # no mistake, through the formulas that take the mistakes


def _row_nll64(row, label, pred, mut):
    """-((z_y - m) - log sum exp(z - m)) of one float64 row, written out so that one of HEAD_ARITHMETIC can be built in.
    m is the maximum that the argmax search found (a NaN where the row holds one, as in the kernel)."""
    C = row.numel()
    seen = row[:64] if mut == "max_first_pass_only" else row
    m = seen.max()                                           # torch.max hands a NaN on
    if mut == "no_max_subtraction":
        m = torch.zeros((), dtype=row.dtype)
    summed = row
    if mut == "lse_first_pass_only":
        summed = row[:64]
    elif mut == "lse_tail_dropped" and C > 64 and C % 64:
        summed = row[:64 * (C // 64)]
    lse = torch.log(torch.exp(summed - m).sum())
    at = label % 64 if mut == "gather_y_mod_64" else pred if mut == "nll_of_pred" else label
    return float(-((row[at] - m) + lse) if mut == "lse_sign" else -((row[at] - m) - lse))


def head64(z, y, rows=None, label_rows=None, ignore_index=-100, mut=None):
    """What eval_head + eval_reduce must give, on the CPU in float64: {"pred", "flag", "counts", "acc", "loss", "nll"}; mut
    None, or one of BOOKKEEPING or HEAD_ARITHMETIC built in.  A row whose logits row, label index or label is outside its
    array is BAD (pred -1 without a logits row); a label equal to ignore_index is IGNORED; acc is over all rows, the loss
    over the others alone.  nll [n] holds each row's term of the loss, 0 for a row that is ignored or bad."""
    z, y = z.double(), y.long()
    n = rows.numel() if rows is not None else label_rows.numel() if label_rows is not None else z.shape[0]
    C = z.shape[1]
    rows = torch.arange(n) if rows is None else rows.long()
    lrows = torch.arange(n) if label_rows is None else label_rows.long()
    pred, flag = torch.full((n,), -1, dtype=torch.int64), torch.full((n,), BAD, dtype=torch.uint8)
    nll = torch.zeros(n, dtype=torch.float64)
    total, n_valid = 0.0, 0
    for i in range(n):
        r, l = int(rows[i]), int(lrows[i])
        if not 0 <= r < z.shape[0]:
            continue
        row = z[r]
        seen = row[:64] if mut == "max_first_pass_only" else row
        nan = torch.isnan(seen)
        if bool(nan.any()) and mut != "nan_not_max":
            pred[i] = int(nan.nonzero()[0])                  # the first NaN, as torch.argmax and numpy
        else:
            v = torch.where(nan, torch.full_like(seen, float("-inf")), seen)
            hits = (v == v.max()).nonzero()[:, 0]
            pred[i] = int(hits[-1] if mut == "tie_last_index" else hits[0])
        if not 0 <= l < y.numel():
            continue
        label = int(y[l])
        if label == ignore_index:
            flag[i] = IGNORED
            if mut == "ignored_in_loss":                      # a head that gathers before it tests the label: class 0
                total, n_valid = total - float(torch.log_softmax(row, dim=0)[0]), n_valid + 1
            continue
        if not 0 <= label < C:
            continue
        flag[i] = CORRECT if int(pred[i]) == label else WRONG
        # torch's own log_softmax unless a mistake goes into it; WRITTEN_OUT is _row_nll64 with none, held to torch's
        # up to the rounding of float64's own sum (tests/test_host_mutants.py)
        written = mut in HEAD_ARITHMETIC or mut == WRITTEN_OUT
        nll[i] = _row_nll64(row, label, int(pred[i]), mut) if written else -float(torch.log_softmax(row, dim=0)[label])
        total += float(nll[i])
    counts = [int((flag <= CORRECT).sum()), int((flag == CORRECT).sum()), int((flag == IGNORED).sum()), int((flag == BAD).sum())]
    n_valid += counts[0]
    den_loss = n if mut == "loss_over_rows" else n_valid
    den_acc = counts[0] if mut == "acc_over_valid" else n
    return {"pred": pred, "flag": flag, "counts": counts, "acc": counts[1] / den_acc if den_acc else float("nan"),
            "loss": total / den_loss if den_loss else float("nan"), "nll": nll}


def head_share(got, ref, loss32, loss_held=True):
    """How far `got` (a head64 result) is from `ref` under the GPU file's assertions: infinite when a quantity the file
    holds exactly differs (pred, flag, counts, acc, a NaN loss), otherwise |loss - loss64| over assert_loss's bound, or 0
    where the file does not look at the loss (`loss_held`)."""
    same = lambda a, b: a == b or (a != a and b != b)  # noqa: E731
    if not (torch.equal(got["pred"], ref["pred"]) and torch.equal(got["flag"], ref["flag"]) and got["counts"] == ref["counts"]
            and same(got["acc"], ref["acc"])):
        return float("inf")
    if not loss_held:
        return 0.0
    if ref["loss"] != ref["loss"] or got["loss"] != got["loss"] or got["loss"] == ref["loss"]:
        return 0.0 if same(got["loss"], ref["loss"]) else float("inf")
    return abs(got["loss"] - ref["loss"]) / (4.0 * abs(loss32 - ref["loss"]) + 2.0 ** -23 * abs(ref["loss"]))


def head_drawn():
    """The head's inputs that tests/test_gpu_evaluate.py draws, up to 65 rows of the grid (the reference walks row by row):
    (name, z, y, {rows, label_rows, ignore_index}, whether the file holds the loss there)."""
    out = [(f"head C={C} n={n}", *head_case(n, C)[:2], {}, True) for C in HEAD_C for n in HEAD_N if n <= 65]
    z, y = ties_case()
    out.append(("ties", z, y, {}, False))
    z, _, y2, rows, lrows, _, _ = ignored_case()
    out.append(("ignored", z, y2, dict(rows=rows, label_rows=lrows), True))
    out.append(("all ignored", z, torch.full((z.shape[0],), 3), dict(ignore_index=3), True))
    return out


REDUCE_N = (0, 1, 1023, 1025, 2047, 2049, 1024 * 5 - 1, 1024 * 1023 + 1, 1024 * 1024 + 1, 1024 * 1025 - 1)
ABSORB_N = 1024 * 5 - 1                                      # the smallest drawn size with more than two slices


def reduce_case(n, seed=0, absorb=False):
    """Synthetic filled buffers (nll float32, flag uint8) and what the reduce must give: (nll, flag, loss64, counts).
    With `absorb` every 1024th row holds 2^24 and the other valid rows 0.75, less than half a float32 ulp of 2^24: the
    float64 sum is exact, a float32 accumulator that has taken the large row in takes in none of the small ones."""
    rng = np.random.default_rng(seed + n)
    flag = rng.integers(0, 4, n).astype(np.uint8)
    nll = (rng.random(n) * 5.0).astype(np.float32)
    if absorb:
        nll[:] = 0.75
        nll[::1024] = 2.0 ** 24
        flag[::1024] = WRONG
    nll[flag >= IGNORED] = 0.0
    counts = [int((flag <= CORRECT).sum()), int((flag == CORRECT).sum()), int((flag == IGNORED).sum()), int((flag == BAD).sum())]
    loss = float(np.sum(nll.astype(np.float64))) / counts[0] if counts[0] else float("nan")
    return torch.from_numpy(nll), torch.from_numpy(flag), loss, counts


def reduce_drawn():
    """What tests/test_gpu_evaluate.py gives the reduce: (name, n, absorb)."""
    return [(f"reduce n={n}", n, False) for n in REDUCE_N] + [(f"reduce n={ABSORB_N} absorb", ABSORB_N, True)]


def reduce64(nll, flag, mut=None):
    """eval_reduce's result from filled buffers, on the CPU: {"loss", "acc", "counts"}, with the kernel's slices (at least
    1024 rows each, at most 1024 of them); mut None, or one of REDUCE_MUTANTS built in."""
    nll, flag = nll.numpy(), flag.numpy()
    n = len(nll)
    grid = min(max(-(-n // 1024), 1), 1024)
    rows = -(-n // grid)                                     # of a slice
    if mut == "reduce_last_slice_dropped":
        nll, flag = nll[:(grid - 1) * rows], flag[:(grid - 1) * rows]
    counts = [int((flag <= CORRECT).sum()), int((flag == CORRECT).sum()), int((flag == IGNORED).sum()), int((flag == BAD).sum())]
    if mut == "reduce_in_float32":                           # numpy's cumsum adds one by one in the dtype it is given
        parts = [np.cumsum(nll[s:s + rows], dtype=np.float32)[-1] for s in range(0, len(nll), max(rows, 1))]
        total = float(np.sum(np.asarray(parts, dtype=np.float64)))
    else:
        total = float(np.sum(nll.astype(np.float64)))
    return {"loss": total / counts[0] if counts[0] else float("nan"), "acc": counts[1] / n if n else float("nan"), "counts": counts}


def reduce_share(got, loss64, counts, n):
    """How far a reduce64 result is from the case under the GPU test's assertions: infinite where the counts, the accuracy
    or a NaN loss differ, otherwise |loss - loss64| over 2^-23 |loss64|."""
    acc = counts[1] / n if n else float("nan")
    same = lambda a, b: a == b or (a != a and b != b)  # noqa: E731
    if got["counts"] != counts or not same(got["acc"], acc) or (got["loss"] != got["loss"]) != (loss64 != loss64):
        return float("inf")
    if loss64 != loss64 or got["loss"] == loss64:
        return 0.0
    return abs(got["loss"] - loss64) / (2.0 ** -23 * abs(loss64))


# ---- the head at its edges: a bound from the kernel's order of operations, that order walked in float32,
# and the drawn cases
U = 2.0 ** -24                                               # half a float32 ulp, relative: one rounding
EDGE_N = 65                                                  # more than one wave per block, one row past 64
EDGE_C = (1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096)       # the lane loop's pass edges, and kMaxC


def bounds64(z, y):
    """row_bound64 for every row of z [n, C] (float32 values, taken as given) with labels y [n] in [0, C): (nll [n], bound
    [n]) in float64.  nll is torch's float64 -log_softmax(z)[y]; the bound is NaN where nll is not finite (such a row is
    held exactly).  With u = 2^-24, m the row's max, t_c = |z_c - m|, p = softmax(z), lse = log sum exp(z_c - m), following
    eval_head_kernel step by step:

        u |z_y - m|                the subtraction z_y - m
      + u sum_c p_c (t_c + 2)      z_c - m rounded (u t_c), then expf (at most 2 ulp = 2u), each by its share of the sum
      + u (ceil(C / 64) + 6)       a lane's serial adds over its passes and the six steps of wave_sum, each at most u of a
                                   partial sum that is at most the whole sum
      + 2u |lse|                   logf, at most 2 ulp of its result
      + 2u |nll|                   the last subtraction and the store

    The 2 ulp of expf and logf are an assumption about the device's library, not a documented figure (DESIGN §7h says
    what the run showed).  A class at -inf has p_c = 0 and contributes nothing; a term whose expf underflows errs by at most
    itself, below 2^-126 of the sum, which the third line covers many times over."""
    z64, y = z.double(), y.long()
    C = z64.shape[1]
    nll = -torch.log_softmax(z64, dim=1).gather(1, y[:, None])[:, 0]
    m = z64.max(dim=1, keepdim=True).values
    t = (z64 - m).abs()
    e = torch.exp(z64 - m)
    s = e.sum(dim=1, keepdim=True)
    spread = torch.where(e > 0, e / s * (t + 2.0), torch.zeros_like(e)).sum(dim=1)
    zy = z64.gather(1, y[:, None])
    bound = U * ((zy - m).abs()[:, 0] + spread + (-(-C // 64) + 6) + 2.0 * torch.log(s)[:, 0].abs() + 2.0 * nll.abs())
    return nll, torch.where(torch.isfinite(nll), bound, torch.full_like(bound, float("nan")))


def row_bound64(z, y):
    """(float64 nll, the largest error a correct float32 head may make) of one row z [C] with label y: see bounds64."""
    nll, bound = bounds64(z[None, :], torch.tensor([int(y)]))
    return float(nll[0]), float(bound[0])


def mean_bound64(nll, bound):
    """(mean64, its bound) of rows that are all finite: mean_i bound_i + 2^-23 |mean64|, the reduce being a float64 sum
    of the float32 rows that is rounded once."""
    mean = float(nll.mean())
    return mean, float(bound.mean()) + 2.0 ** -23 * abs(mean)


def head_walk32(z, y):
    """eval_head_kernel's order in numpy float32 for the rows of z [n, C] and labels y [n] in [0, C): float32 [n].  Class
    c goes to lane c % 64 and is added pass by pass into that lane's accumulator, the 64 accumulators go through the xor
    tree 32 ... 1, then logf and -((z_y - max) - ls).  numpy's float32 exp and log stand in for expf and logf.  The lanes
    past C add exp(-inf - max) = 0 here, where the kernel adds nothing: the same bits."""
    z, y = z.numpy().astype(np.float32), y.numpy()
    n, C = z.shape
    passes = -(-C // 64)
    padded = np.full((n, passes * 64), -np.inf, dtype=np.float32)
    padded[:, :C] = z
    lane = np.arange(64)
    with np.errstate(all="ignore"):
        best = z.max(axis=1)                                 # a NaN in the row is its max, as in the kernel's search
        e = np.zeros((n, 64), dtype=np.float32)
        for k in range(passes):
            e = e + np.exp(padded[:, 64 * k:64 * k + 64] - best[:, None])
        for o in (32, 16, 8, 4, 2, 1):
            e = e + e[:, lane ^ o]
        out = -((z[np.arange(n), y] - best) - np.log(e[:, 0]))
    assert out.dtype == np.float32
    return out


def _rotation(z):
    """Labels by a fixed rotation over the rows: 0, C-1, min(63, C-1), min(64, C-1), min(65, C-1), the argmax, the argmin
    (of the finite classes), so that y >= 64, y = C-1, the correct and the most wrong class all occur.  A label that lands
    on a -inf class moves one class down (the masked classes are every third one, never class 0)."""
    n, C = z.shape
    top = torch.argmax(z, dim=1)
    low = torch.argmin(torch.where(torch.isfinite(z), z, torch.full_like(z, float("inf"))), dim=1)
    y = torch.empty(n, dtype=torch.int64)
    for i in range(n):
        y[i] = (0, C - 1, min(63, C - 1), min(64, C - 1), min(65, C - 1), int(top[i]), int(low[i]))[i % 7]
        if z[i, y[i]] == float("-inf"):
            y[i] -= 1
    return y


def _masked(z):
    z = z.clone()
    z[:, 2::3] = float("-inf")
    return z


def _edge_drawn():
    out = []
    for ci, C in enumerate(EDGE_C):
        def g(family):
            return torch.Generator().manual_seed(7000 + 100 * family + ci)
        n = EDGE_N
        wide = torch.randn((n, C), generator=g(0)) * 30.0
        out.append((f"wide C={C}", wide, _rotation(wide), {}))
        huge = torch.randn((n, C), generator=g(1)) * 1e4 + 1e6
        out.append((f"huge C={C}", huge, _rotation(huge), {}))
        conf = torch.randn((n, C), generator=g(2)) - 30.0
        y = _rotation(conf)
        conf[torch.arange(n), y] = 0.0
        out.append((f"confident C={C}", conf, y, {}))
        flat = torch.full((n, C), 5.0)
        out.append((f"flat C={C}", flat, _rotation(flat), {}))
        zeros = torch.where(torch.rand((n, C), generator=g(3)) < 0.5, -0.0, 0.0)
        zeros[::2, 0] = -0.0                                 # a -0.0 first, a 0.0 after it: still index 0
        zeros[::2, C // 2] = 0.0
        out.append((f"flat signed zeros C={C}", zeros, _rotation(zeros), {}))
        if C >= 3:
            masked = _masked(torch.randn((n, C), generator=g(4)) * 3.0)
            ym = _rotation(masked)
            out.append((f"masked C={C}", masked, ym, {}))
        if C >= 65:                                          # class 64 has to exist
            z, y = masked.clone(), ym.clone()
            y[5] = C - 1 - (C - 3) % 3                       # the last -inf class: nll = +inf
            z[17, C - 1], y[17] = float("inf"), 0            # inf - inf: NaN
            z[40, 64], y[40] = float("nan"), 1               # a NaN is the max: NaN
            z[64, :], y[64] = float("-inf"), 0               # -inf - -inf: NaN, and pred = label = 0
            out.append((f"special C={C}", z, y, {}))
    C, R, n = 4096, 300, 200
    gen = torch.Generator().manual_seed(7999)
    z = torch.randn((R, C), generator=gen) * 30.0
    rows = torch.randint(0, R, (n,), generator=gen)
    rows[:40] = torch.arange(R - 1, R - 41, -1)              # reverse order
    rows[40:60] = 17                                         # duplicates
    lrows = torch.randint(0, R, (n,), generator=gen)         # labels picked by another list
    out.append(("gathered4096", z, _rotation(z), dict(rows=rows, label_rows=lrows)))
    return out


# (name, z, y, {rows, label_rows}): built once, read by tests/test_gpu_evaluate_edges.py and tests/test_host_mutants.py;
# nothing that reads them modifies them.  Every label is in [0, C) and every index inside its array.
EDGE_DRAWN = _edge_drawn()
EDGE_NAMES = [c[0] for c in EDGE_DRAWN]
EDGE_SPECIAL_ROWS = (5, 17, 40, 64)                          # of the `special` cases: +inf, NaN, NaN, NaN
PRINT_ONLY = ("huge", "flat")                                # families where torch's float32 can be exact: §7g's rule is printed


def edge_family(name):
    return name.split(" C=")[0]


@functools.lru_cache(maxsize=None)
def edge_reference(name):
    """What a case of EDGE_DRAWN must give, from torch on the CPU, computed once: the gathered logits and labels (zz, yy),
    pred, flag, counts, acc, and nll64 with its bound per row (bounds64)."""
    _, z, y, kw = EDGE_DRAWN[EDGE_NAMES.index(name)]
    n = kw["rows"].numel() if "rows" in kw else z.shape[0]
    zz, yy = z[kw.get("rows", torch.arange(n))], y[kw.get("label_rows", torch.arange(n))]
    pred = torch.argmax(zz, dim=1)
    nll, bound = bounds64(zz, yy)
    n_correct = int((pred == yy).sum())
    return {"zz": zz, "yy": yy, "pred": pred, "flag": (pred == yy).to(torch.uint8), "counts": [n, n_correct, 0, 0],
            "acc": float(np.float32(n_correct / n)), "nll": nll, "bound": bound, "mean": float(nll64(zz, yy))}


def edge_share(got, ref, bound):
    """How far `got` (a head64 result) is from `ref` under tests/test_gpu_evaluate_edges.py's assertions: infinite where
    a quantity held exactly differs (pred, flag, counts, acc, a row that is not finite), otherwise the largest
    |nll_i - nll64_i| / bound_i."""
    same = lambda a, b: a == b or (a != a and b != b)  # noqa: E731
    a, b = got["nll"], ref["nll"]
    fin = torch.isfinite(b)
    if not (torch.equal(got["pred"], ref["pred"]) and torch.equal(got["flag"], ref["flag"]) and got["counts"] == ref["counts"]
            and same(got["acc"], ref["acc"]) and torch.equal(torch.isfinite(a), fin)
            and torch.equal(torch.nan_to_num(a[~fin], nan=1.0), torch.nan_to_num(b[~fin], nan=1.0))):
        return float("inf")
    return float(((a - b).abs()[fin] / bound[fin]).max()) if bool(fin.any()) else 0.0


def features(n_nodes, seed=3):
    """Bag-of-words like node features, 5 % non-zero, of either sign: the rows' average carries no common offset that
    would send every node to the same class."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((n_nodes, F_IN), generator=g) < 0.05).float() * torch.sign(torch.randn((n_nodes, F_IN), generator=g))


def node_labels(n_nodes, seed=4):
    return torch.randint(0, CLASSES, (n_nodes,), generator=torch.Generator().manual_seed(seed))


def model_pair(name, seed=11, f_in=F_IN, small=False):
    """(GrandPlusMLP on the CPU, its float64 restatement), equal parameters, non-trivial BatchNorm state; with `small`,
    infer_cases.small_var's running variances and per-layer epsilons."""
    from grand_plus_amd.mlp import GrandPlusMLP
    use_bn, norm = MODELS[name]
    torch.manual_seed(seed)
    ours = GrandPlusMLP(f_in, CLASSES, HIDDEN, LAYERS, use_bn, 0.5, 0.7, norm)
    g = torch.Generator().manual_seed(seed + 1)
    for b in ours.bns:
        b.weight.data = torch.rand(b.weight.shape, generator=g) + 0.5
        b.bias.data = torch.randn(b.bias.shape, generator=g) * 0.01
        b.running_mean.data = torch.randn(b.running_mean.shape, generator=g) * 0.01
        b.running_var.data = torch.rand(b.running_var.shape, generator=g) + 0.5
    ours.fcs[0].weight.data *= FIRST_SCALE
    ours.fcs[-1].weight.data *= LAST_SCALE
    ref = RefMLP(f_in, CLASSES, HIDDEN, LAYERS, use_bn, 0.5, 0.7, norm)
    ref.load_state_dict(ours.state_dict())
    if small:
        from infer_cases import small_var
        small_var(ours, ref)
    return ours, ref.double().eval()


def chain64(ref, x64, y):
    """The float64 end of both chains on the CPU: logits of the restatement in eval mode on x64, then what the tests hold
    ours against.  Returns a dict:
      loss, pred      float64 nll_loss and argmax;
      dz [n]          per row, the largest error the MLP test (tests/test_gpu_mlp.py) allows a logit of ours:
                      max_c 2e-5 * (|a| |W|^T + |b|)_c + 1e-6, a = the last Linear's input;
      loss_bound      log-softmax moves by at most 2 max_c |dz_c| per row (log-sum-exp is 1-Lipschitz in the sup norm, and
                      z_y moves by at most the same), so the mean moves by at most mean_i 2 dz_i; the head's own fp32
                      arithmetic (z - max, log of the sum, the final subtraction: three roundings of at most 2 ulp) adds
                      at most 2^-22 * mean_i (|z_y - max| + |log sum|);
      decided [n]     rows whose float64 top-2 gap exceeds 2 dz_i: no logits within the bound can change their argmax."""
    with torch.no_grad():
        z = ref(x64, None)
        fc = ref.fcs[-1]
        scale = ref.last_a.abs() @ fc.weight.abs().t() + fc.bias.abs()
    dz = (2e-5 * scale + 1e-6).max(dim=1).values
    top2 = torch.topk(z, 2, dim=1).values if z.shape[1] > 1 else torch.cat([z, z - 1.0], dim=1)
    m = z.max(dim=1).values
    lse = torch.log(torch.exp(z - m[:, None]).sum(dim=1))
    zy = z.gather(1, y[:, None])[:, 0]
    head = 2.0 ** -22 * float(((zy - m).abs() + lse.abs()).mean())
    sup = grand_loss_ref([z], y, y.numel(), 0.0, 1.0, 0.0, "l2")[1]      # the supervised term of the objective's restatement
    return {"loss": float(sup), "pred": z.argmax(dim=1), "dz": dz,
            "loss_bound": float((2.0 * dz).mean()) + head, "decided": (top2[:, 0] - top2[:, 1]) > 2.0 * dz}


def valid64(ref, X, col, val, filled, K, positions, y):
    """The reference's valid() in float64: random_prop (eval mode) over the rows at `positions`, then chain64."""
    idx, cols, scores, _ = rows_to_coo(col, val, filled, K, positions)
    n_out = positions.numel()
    if int(idx[-1]) + 1 != n_out:                         # random_prop_ref sizes its output by the last entry
        raise ValueError("the last row of the batch is empty")
    aug = random_prop_ref(X.double()[cols], scores.double(), idx, 0.5, False)
    return chain64(ref, aug, y)


def predict64(ref, adj, X, mode, order, alpha, idx, y):
    """The reference's predict() in float64 on the rows idx."""
    prop = torch.from_numpy(propagate_ref(adj, X.numpy(), mode, order, alpha))
    return chain64(ref, prop[idx], y)


def assert_decided_preds(pred, r64, what):
    """At most LEFT_OUT of the rows may be undecided in float64 (asserted first); on every other row pred must match."""
    left_out = 1.0 - float(r64["decided"].double().mean())
    print(f"[evaluate] {what}: {left_out:.4f} of the rows within the margin")
    assert left_out <= LEFT_OUT, (what, left_out)
    d = r64["decided"]
    assert torch.equal(pred.cpu().long()[d], r64["pred"][d]), what
