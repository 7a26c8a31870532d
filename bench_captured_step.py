#!/usr/bin/env python3
"""bench_captured_step.py -- a whole GRAND+ training step, eager against captured, one JSON line per case.

Not the driver's bench (that is bench.py = GFPush rows/s).  At the cora, reddit and amazon2m step shapes of
bench_mlp_step.py, S = 2, three variants of one step (select a batch -> random_prop_rows -> MLP -> loss -> backward ->
clip + Adam), alternated window by window in one process:
  eager     today's composition with host numbers: a host seed for random_prop_rows and the MLP, the host weight of
            model.py:329, ClipAdam with its host step count
  twin      TrainStep(capture=False): the same kernels fed by gp_step_advance / gp_step_masks, run eagerly
  replay    TrainStep(capture=True): one graph replay per step
Every variant gets a fresh selection per step from the same pre-drawn list and uploads it the same way.
Per variant: `<v>_us` GPU time per step (CUDA events around a window of --iters steps, median of --reps windows) and
`<v>_host_us`, the host wall clock per step to enqueue the same window (what the capture removes).
--profile-variant <case>:<variant> runs that one variant for --iters steps after its warm-up, for a rocprofv3
--kernel-trace --stats run of its own (the mask launch's share is read off step_masks_kernel there).

Features, rows and labels are synthetic (uniform random neighbours and scores).
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
from bench_mlp_step import CASES, P_NODE, S, TEM  # noqa: E402
from grand_plus_amd import ClipAdam, StepState, TrainStep  # noqa: E402
from grand_plus_amd._common import step_seed  # noqa: E402
from grand_plus_amd.augment import random_prop_rows  # noqa: E402
from grand_plus_amd.mlp import GrandPlusMLP  # noqa: E402
from grand_plus_amd.objective import grand_plus_loss  # noqa: E402
from grand_plus_amd.rows import RowMatrix  # noqa: E402
from grand_plus_amd.step import step_weight, trained_parameters  # noqa: E402

STEP_CASES = ("cora", "reddit", "amazon2m")
LAM, WARMUP, BASE_SEED, N_SELECTIONS = 1.0, 100, 0x5EED, 64
ADAM = dict(lr=1e-2, weight_decay=5e-4, clip_norm=0.1)


def build(name, dev, rng):
    _layout, F, H, C, nl, bn, pin, phid, n_l, n_u, (N, K, kind) = CASES[name]
    S_rows = min(20_000, N)
    seeds = rng.choice(N, S_rows, replace=False).astype(np.int64)
    col, val, filled = synthetic_rows(rng, dev, S_rows, K, N)
    row = torch.from_numpy(np.repeat(seeds, K).astype(np.int32)).to(dev)
    rm = RowMatrix(seeds, K, row, col, val, filled, N)
    n_train = S_rows // 10
    sels = [(rng.choice(n_train, n_l, replace=False), rng.choice(S_rows - n_train, n_u, replace=False))
            for _ in range(N_SELECTIONS)]
    return dict(name=name, rm=rm, X=torch.randn((N, F), device=dev), labels=torch.from_numpy(rng.integers(0, C, N)).to(dev),
                idx_train=seeds[:n_train], idx_unlabel=seeds[n_train:], n_train=n_train, sels=sels, n_l=n_l, kind=kind,
                model_args=(F, C, H, nl, bn, pin, phid, bn))


def make_model(c, dev):
    torch.manual_seed(0)
    return GrandPlusMLP(*c["model_args"]).to(dev).train()


def variants(c, dev):
    """name -> step(i): one training step on the i-th selection."""
    rm, X, n_l, kind = c["rm"], c["X"], c["n_l"], c["kind"]
    out = {}

    m = make_model(c, dev)
    opt = ClipAdam(trained_parameters(m), **ADAM)
    pos = rm.batch_positions(np.concatenate([c["idx_train"], c["idx_unlabel"]]), check=True)
    pool_labels = c["labels"][torch.from_numpy(c["idx_train"]).to(dev)]
    tick = [0]

    def eager(i):
        tr, un = c["sels"][i % N_SELECTIONS]
        sel = torch.from_numpy(np.concatenate([tr, un + c["n_train"]])).pin_memory().to(dev, non_blocking=True)
        tick[0] += 1
        seed, w = step_seed(BASE_SEED, tick[0]), float(step_weight(LAM, WARMUP, tick[0]))
        opt.zero_grad(set_to_none=True)
        aug = random_prop_rows(X, rm.col, rm.val, rm.filled, rm.K, batch_rows=pos.index_select(0, sel), dropnode_rate=P_NODE,
                               training=True, seed=seed, samples=S)
        loss, _ = grand_plus_loss(m(aug, seed=seed), pool_labels.index_select(0, sel[:n_l]), n_l, w, tem=TEM, kind=kind)
        loss.backward()
        opt.step()

    out["eager"] = eager
    for key, capture in (("twin", False), ("replay", True)):
        mm = make_model(c, dev)
        ts = TrainStep(mm, ClipAdam(trained_parameters(mm), capturable=True, state=StepState(dev), **ADAM), rm, X, c["labels"], c["idx_train"],
                       c["idx_unlabel"], samples=S, dropnode_rate=P_NODE, lam=LAM, warmup=WARMUP, tem=TEM, kind=kind,
                       seed=BASE_SEED, capture=capture)
        out[key] = lambda i, ts=ts: ts.step(*c["sels"][i % N_SELECTIONS])
    return out


def window(fn, iters, start):
    """(GPU microseconds, host microseconds) per step over one window of `iters` steps."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for i in range(iters):
        fn(start + i)
    b.record()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3, host / iters * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(STEP_CASES))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--profile-variant", default=None, help="<case>:<variant>: warm it up, then run it --iters times")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    if a.profile_variant:
        name, var = a.profile_variant.split(":")
        fn = variants(build(name, dev, rng), dev)[var]
        for i in range(3 + a.iters):
            fn(i)
        torch.cuda.synchronize()
        return
    for name in a.cases.split(","):
        c = build(name, dev, rng)
        v = variants(c, dev)
        for fn in v.values():                                       # warm-up: code load, optimiser state, the capture
            for i in range(3):
                fn(i)
        torch.cuda.synchronize()
        gpu = {k: [] for k in v}
        host = {k: [] for k in v}
        for rep in range(a.reps):
            for k, fn in v.items():                                 # alternated: a drift of the clocks reaches all three
                g, h = window(fn, a.iters, 3 + rep * a.iters)
                gpu[k].append(g)
                host[k].append(h)
        _layout, F, H, C, nl, bn, pin, phid, n_l, n_u, _step = CASES[name]
        rec = {"case": name, "S": S, "B": n_l + n_u, "F": F, "H": H, "C": C, "nlayers": nl, "bn_norm": bn,
               "dropout": [pin, phid], "iters": a.iters, "reps": a.reps}
        for k in v:
            rec[k + "_us"] = round(float(np.median(gpu[k])), 1)
            rec[k + "_us_range"] = [round(min(gpu[k]), 1), round(max(gpu[k]), 1)]
            rec[k + "_host_us"] = round(float(np.median(host[k])), 1)
        rec["replay_speedup_vs_eager"] = round(rec["eager_us"] / rec["replay_us"], 2)
        rec["replay_speedup_vs_twin"] = round(rec["twin_us"] / rec["replay_us"], 2)
        emit(rec, a.out)


if __name__ == "__main__":
    main()
