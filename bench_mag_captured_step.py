#!/usr/bin/env python3
"""bench_mag_captured_step.py -- a whole MAG training step, eager against captured, one JSON line.

Not the driver's bench (that is bench.py = GFPush rows/s).  At bench_mag_rows.py's mag-train shape (V = 500 000, H = 64,
B = 40, K = 32, S = 2, synthetic bags of mean 20, 2 000 000 nodes, input_droprate 0), seven variants of one step (select a
batch -> emb_rows -> MagMLP -> loss -> backward -> clip + Adam over the table and the layers), alternated window by window in
one process:
  eager           what the project offered before MagTrainStep: emb_rows + MagMLP + grand_plus_loss + ClipAdam.step() with
                  host numbers (a host seed, the host weight of model.py:329, ClipAdam's host step count); atomic dW
  replay-atomic   MagTrainStep(capture=True, deterministic=False): one graph replay per step, atomic dW
  replay-det      MagTrainStep(capture=True, deterministic=True): the same with the sort-then-gather dW of mag_det
  replay-det-exact  replay-det with table_step="exact" (DESIGN §7t): the table stepped from the backward's row list, bit for
                  bit replay-det's update, without the zero-fill of dW and its two dense reads
  replay-det-lazy   replay-det with table_step="lazy": the touched rows of the table and its moments alone -- NOT the reference's
                  dense Adam; the table sits in a parameter group of its own with weight_decay = 0, which lazy mode requires
  replay-atomic-exact, replay-atomic-lazy   replay-atomic with row_list="bitmap"  and the same two table steps:
                  the rows are listed from a bitmap, no sort and no gather, and dW is zeroed on the listed rows alone
Every variant gets a fresh selection per step from the same pre-drawn list and uploads it the same way.
Per variant: `<v>_us` wall clock per step (a window of --iters steps between two synchronisations, median [min, max] of
--reps windows) and `<v>_host_us`, the host time per step to enqueue the same window.
--profile-variant <variant> runs that one variant for --iters steps after its warm-up, for a rocprofv3 --kernel-trace --stats
run of its own (the sort's share of replay-det is read off there).

The attribute CSR, the table, the rows and the labels are synthetic (uniform random neighbours, scores and attributes).
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from _bench_steps import emit, synthetic_rows  # noqa: E402
from grand_plus_amd import ClipAdam, MagTrainStep, StepState, mag_trained_parameters  # noqa: E402
from grand_plus_amd._common import step_seed  # noqa: E402
from grand_plus_amd.mlp import MagMLP  # noqa: E402
from grand_plus_amd.objective import grand_plus_loss  # noqa: E402
from grand_plus_amd.rows import RowMatrix  # noqa: E402
from grand_plus_amd.step import step_weight  # noqa: E402

S, P_NODE, TEM, C, N_L, N_U = 2, 0.5, 0.5, 8, 20, 20
LAM, WARMUP, BASE_SEED, N_SELECTIONS = 1.0, 100, 0x5EED, 64
ADAM = dict(lr=1e-2, weight_decay=5e-4, clip_norm=0.1)
VARIANTS = ("eager", "replay-atomic", "replay-det", "replay-det-exact", "replay-det-lazy", "replay-atomic-exact", "replay-atomic-lazy")


def build(a, dev):
    rng = np.random.default_rng(0)
    N, V, K = a.nodes, a.vocab, a.K
    lens = rng.integers(1, 2 * a.bag, N)
    indptr = np.zeros(N + 1, np.int64)
    np.cumsum(lens, out=indptr[1:])
    indices = rng.integers(0, V, int(indptr[-1])).astype(np.int32)
    data = (rng.random(int(indptr[-1]), dtype=np.float32) + 0.05).astype(np.float32)
    attrs = tuple(torch.from_numpy(x).to(dev) for x in (indptr, indices, data))
    S_rows = 20_000
    seeds = rng.choice(N, S_rows, replace=False).astype(np.int64)
    col, val, filled = synthetic_rows(rng, dev, S_rows, K, N)
    row = torch.from_numpy(np.repeat(seeds, K).astype(np.int32)).to(dev)
    rm = RowMatrix(seeds, K, row, col, val, filled, N)
    n_train = S_rows // 10
    sels = [(rng.choice(n_train, N_L, replace=False), rng.choice(S_rows - n_train, N_U, replace=False)) for _ in range(N_SELECTIONS)]
    return dict(rm=rm, attrs=attrs, labels=torch.from_numpy(rng.integers(0, C, N)).to(dev), idx_train=seeds[:n_train],
                idx_unlabel=seeds[n_train:], n_train=n_train, sels=sels, model_args=(V, C, a.hidden, 2, True, 0.0, 0.5, True))


def make_model(c, dev):
    torch.manual_seed(0)
    return MagMLP(*c["model_args"]).to(dev).train()


def variants(c, dev, only=None):
    """name -> step(i): one training step on the i-th selection."""
    rm, attrs = c["rm"], c["attrs"]
    out = {}
    if only in (None, "eager"):
        m = make_model(c, dev)
        opt = ClipAdam(mag_trained_parameters(m), **ADAM)
        pos = rm.batch_positions(np.concatenate([c["idx_train"], c["idx_unlabel"]]), check=True)
        pool_labels = c["labels"][torch.from_numpy(c["idx_train"]).to(dev)]
        tick = [0]

        def eager(i):
            tr, un = c["sels"][i % N_SELECTIONS]
            sel = torch.from_numpy(np.concatenate([tr, un + c["n_train"]])).pin_memory().to(dev, non_blocking=True)
            tick[0] += 1
            seed, w = step_seed(BASE_SEED, tick[0]), float(step_weight(LAM, WARMUP, tick[0]))
            opt.zero_grad(set_to_none=True)
            aug = m.emb_rows(*attrs, rm, batch_rows=pos.index_select(0, sel), samples=S, dropnode_rate=P_NODE, seed=seed)
            loss, _ = grand_plus_loss(m(aug, seed=seed), pool_labels.index_select(0, sel[:N_L]), N_L, w, tem=TEM, kind="l2")
            loss.backward()
            opt.step()

        out["eager"] = eager
    for key, det, table_step in (("replay-atomic", False, None), ("replay-det", True, None), ("replay-det-exact", True, "exact"),
                                 ("replay-det-lazy", True, "lazy"), ("replay-atomic-exact", False, "exact"),
                                 ("replay-atomic-lazy", False, "lazy")):
        if only not in (None, key):
            continue
        mm = make_model(c, dev)
        params = mag_trained_parameters(mm)
        if table_step == "lazy":                                    # lazy mode takes no weight decay on the table
            params = [dict(params=params[:1], weight_decay=0.0), dict(params=params[1:])]
        kw = {} if table_step is None else dict(table_step=table_step)
        if table_step is not None and not det:                      # the atomic backward's row list
            kw["row_list"] = "bitmap"
        ts = MagTrainStep(mm, ClipAdam(params, capturable=True, state=StepState(dev), **ADAM), rm, *attrs,
                          c["labels"], c["idx_train"], c["idx_unlabel"], samples=S, dropnode_rate=P_NODE, lam=LAM, warmup=WARMUP,
                          tem=TEM, kind="l2", seed=BASE_SEED, capture=True, deterministic=det, **kw)
        out[key] = lambda i, ts=ts: ts.step(*c["sels"][i % N_SELECTIONS])
        out[key].step = ts
    return out


def window(fn, iters, start):
    """(wall microseconds, host microseconds) per step over one window of `iters` steps."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(iters):
        fn(start + i)
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6, host / iters * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=2_000_000)
    ap.add_argument("--vocab", type=int, default=500_000)
    ap.add_argument("--bag", type=int, default=20, help="attributes per node (each node gets 1 .. 2*bag-1, mean bag)")
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--K", type=int, default=32)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    ap.add_argument("--profile-variant", default=None, choices=VARIANTS, help="warm it up, then run it --iters times")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    c = build(a, dev)
    v = variants(c, dev, a.profile_variant)
    for fn in v.values():                                           # warm-up: code load, optimiser state, the capture
        for i in range(3):
            fn(i)
    torch.cuda.synchronize()
    if a.profile_variant:
        for i in range(a.iters):
            v[a.profile_variant](3 + i)
        torch.cuda.synchronize()
        return
    wall = {k: [] for k in v}
    host = {k: [] for k in v}
    for rep in range(a.reps):
        for k, fn in v.items():                                     # alternated: a drift of the clocks reaches every variant
            w, h = window(fn, a.iters, 3 + rep * a.iters)
            wall[k].append(w)
            host[k].append(h)
    det = v["replay-det"].step
    for k in v:
        if k != "eager":
            v[k].step.check_entries_flag()
    rec = {"case": "mag-train-step", "S": S, "B": N_L + N_U, "K": a.K, "H": a.hidden, "C": C, "assumed_vocab": a.vocab,
           "assumed_bag_mean": a.bag, "assumed_nodes": a.nodes, "longest_bag": det.longest_bag,
           "max_entries": det._max_entries(N_L + N_U), "table_bytes": 4 * a.vocab * a.hidden, "iters": a.iters, "reps": a.reps}
    for k in v:
        key = k.replace("-", "_")
        rec[key + "_us"] = round(float(np.median(wall[k])), 1)
        rec[key + "_us_range"] = [round(min(wall[k]), 1), round(max(wall[k]), 1)]
        rec[key + "_host_us"] = round(float(np.median(host[k])), 1)
        rec[key + "_host_us_range"] = [round(min(host[k]), 1), round(max(host[k]), 1)]
    emit(rec, a.out)


if __name__ == "__main__":
    main()
