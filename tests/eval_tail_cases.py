"""Cases and numpy mirrors of the fused evaluation tail, shared by tests/test_host_eval_tail.py and
tests/test_gpu_eval_tail.py: the slice plan of csrc/eval_plan.hpp, the reduction of eval_reduce_kernel / eval_tail_kernel in
the kernels' own order of additions (so that its float32 results are the GPU's bits), the deliberate mistakes of §7q's
method, and the drawn inputs."""
import numpy as np
import torch

WRONG, CORRECT, IGNORED, BAD = 0, 1, 2, 3
BLOCK, WAVES = 256, 4
SLOTS, MIN_SLICE = 1024, 1024
TAIL_SLICES = 64
TAIL_MAX_ROWS = TAIL_SLICES * MIN_SLICE
TAIL_WORKSPACE_BYTES = 64
PLAN_N = (0, 1, 1023, 1024, 1025, 2048, 2049, 65535, 65536)

# the mistakes the cases have to tell from the right answer:
#   slice_unclamped      the slice taken as ceil(n / 1024) -- n over the most slots, the grid not clamped to what n needs --
#                        while the right number of slices is walked: rows past grid * slice are never summed
#   float32_accumulation the per-thread sums, the trees and the slots in float32
#   slot_order           a thread's four slots summed q0 + (q1 + (q2 + q3))
#   acc_over_valid       the accuracy divided by n_valid, not by n
MISTAKES = ("slice_unclamped", "float32_accumulation", "slot_order", "acc_over_valid")


def plan(n, mistake=None):
    """(grid, slice) of csrc/eval_plan.hpp's reduce_plan."""
    grid = min(max(-(-n // MIN_SLICE), 1), SLOTS)
    if mistake == "slice_unclamped":
        return grid, -(-n // SLOTS)
    return grid, -(-n // grid)


def _block_sum(v):
    """gp_common.hpp's block_sum over the 256 values of a workgroup: the xor butterfly inside each wave, then the waves in order."""
    v = v.reshape(WAVES, 64).copy()
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
    s = v[0, 0]
    for w in range(1, WAVES):
        s = s + v[w, 0]
    return s


def _thread_sums(x, dtype):
    """Thread tid's sum of x[tid], x[tid + 256], ... in order, from 0."""
    s = np.zeros(BLOCK, dtype=dtype)
    pad = np.zeros(-(-max(len(x), 1) // BLOCK) * BLOCK, dtype=dtype)
    pad[:len(x)] = x
    for row in pad.reshape(-1, BLOCK):
        s = s + row
    return s


def reduce_mirror(nll, flag, mistake=None):
    """What gp_eval_reduce and gp_eval_tail write for filled buffers, in their order of additions: (loss, acc) as numpy
    float32, the four counts, and the float64 sum the loss is the quotient of -- the kernels never store it, but it is where
    the order of the additions shows: the float32 quotient hides a last-bit difference of the sum but at a rounding tie.
    nll float32 [n], flag uint8 [n] (numpy)."""
    nll, flag = np.asarray(nll, dtype=np.float32), np.asarray(flag, dtype=np.uint8)
    n = len(nll)
    acc_t = np.float32 if mistake == "float32_accumulation" else np.float64
    grid, rows = plan(n, mistake)
    slots = np.zeros(SLOTS, dtype=acc_t)
    counts = np.zeros(4, dtype=np.int64)
    with np.errstate(all="ignore"):
        for b in range(grid):
            first, last = b * rows, min(n, (b + 1) * rows)
            slots[b] = _block_sum(_thread_sums(nll[first:last].astype(acc_t), acc_t))
            f = flag[first:last]
            counts += np.array([(f <= CORRECT).sum(), (f == CORRECT).sum(), (f == IGNORED).sum(), (f == BAD).sum()], dtype=np.int64)
        q = slots.reshape(BLOCK, 4)
        per_thread = q[:, 0] + (q[:, 1] + (q[:, 2] + q[:, 3])) if mistake == "slot_order" else ((q[:, 0] + q[:, 1]) + q[:, 2]) + q[:, 3]
        s = np.float64(_block_sum(per_thread))
        loss = np.float32(s / np.float64(counts[0]))
        acc = np.float32(np.float64(counts[1]) / np.float64(counts[0] if mistake == "acc_over_valid" else n))
    return loss, acc, [int(c) for c in counts], s


def bits(x):
    """The bit pattern of a float32 (a NaN compares by its bits)."""
    return int(np.asarray(x, dtype=np.float32).view(np.uint32))


def same(a, b, sum64=True):
    """Two results of reduce_mirror (or the GPU's loss, acc, counts with sum64=False) bit for bit."""
    return bits(a[0]) == bits(b[0]) and bits(a[1]) == bits(b[1]) and list(a[2]) == list(b[2]) and \
        (not sum64 or np.float64(a[3]).view(np.uint64) == np.float64(b[3]).view(np.uint64))


# ---- filled buffers for the mirror
def spread_nll(n, seed=5):
    """nll values spread log-uniformly over 1e-6 ... 1e3: the order of the float64 additions shows in the sum."""
    rng = np.random.default_rng(seed + n)
    return (10.0 ** rng.uniform(-6.0, 3.0, n)).astype(np.float32)


SPREAD_N = 4097                                              # five slices: thread 0 of stage 2 adds four slots, thread 1 one


def buffer_cases():
    """name -> (nll, flag): every flag kind present, sizes on both sides of a slice edge, the spread sums, a float32 trap."""
    rng = np.random.default_rng(17)
    out = {}
    for n in (1, 5, 1025, 2049, SPREAD_N):
        flag = rng.integers(0, 4, n).astype(np.uint8)
        flag[:min(n, 4)] = np.arange(4)[:min(n, 4)]
        nll = spread_nll(n)
        nll[flag >= IGNORED] = 0.0
        out[f"spread{n}"] = (nll, flag)
    n = 2049                                                  # 2^24 then 0.75s: a float32 accumulator takes none of them in
    nll = np.full(n, 0.75, dtype=np.float32)
    nll[::1024] = 2.0 ** 24
    out["absorb"] = (nll, np.full(n, WRONG, dtype=np.uint8))
    out["all_ignored"] = (np.zeros(7, dtype=np.float32), np.full(7, IGNORED, dtype=np.uint8))
    out["empty"] = (np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.uint8))
    return out


# ---- inputs for the GPU: logits and labels whose head gives a chosen nll
def spread_logits(n, seed=5):
    """(logits float32 [n, 2], labels int64 [n]) whose nll is close to spread_nll(n, seed): row i has logits (0, d) and the
    label that makes -log softmax about the target, log(1 + exp(-|d|)) below log 2 and about |d| above it."""
    t = spread_nll(n, seed).astype(np.float64)
    small = t < 0.69
    d = np.where(small, -np.log(np.expm1(np.minimum(t, 0.69))), t + np.log1p(-np.exp(-np.maximum(t, 0.69))))
    z = np.zeros((n, 2), dtype=np.float32)
    z[:, 1] = d
    labels = np.where(small, 1, 0).astype(np.int64)          # small: the label is the larger logit (d > 0 there)
    return torch.from_numpy(z), torch.from_numpy(labels)


def mixed_case(n, C, seed=0, n_labels=None):
    """(logits [n, C], labels [n_labels]) with the label mix of the issue: ignored labels, labels outside [0, C), a NaN
    logit, a row of equal logits; n_labels defaults to n."""
    rng = np.random.default_rng(seed + 1000 * n + C)
    z = (rng.standard_normal((n, C)) * 3.0).astype(np.float32)
    m = n if n_labels is None else n_labels
    y = rng.integers(0, C, m).astype(np.int64)
    k = min(n, m)
    y[:k:4] = np.argmax(z[:k:4], axis=1)                      # every fourth label is its row's argmax: correct rows at every C
    if m > 0:
        y[rng.random(m) < 0.15] = -100
        y[rng.random(m) < 0.05] = C
        y[rng.random(m) < 0.05] = -1
    if n > 2:
        z[1, rng.integers(0, C)] = np.nan
        z[2, :] = 0.5
    return torch.from_numpy(z), torch.from_numpy(y)


def index_lists(n, n_logit_rows, n_labels, seed=0):
    """(rows, label_rows) int64 [n]: mostly in range, some indices outside their arrays on both sides."""
    rng = np.random.default_rng(seed + n)
    rows = rng.integers(0, max(n_logit_rows, 1), n).astype(np.int64)
    lrows = rng.integers(0, max(n_labels, 1), n).astype(np.int64)
    if n > 4:
        rows[0], rows[3] = -1, n_logit_rows
        lrows[1], lrows[4] = n_labels, -7
    return torch.from_numpy(rows), torch.from_numpy(lrows)
