#!/usr/bin/env python3
"""bench_fit.py -- the training loop around a captured GRAND+ step, host-driven against `fit`, one JSON
line per case.

Not the driver's bench (that is bench.py = GFPush rows/s).  At the cora, reddit and amazon2m step shapes of
bench_mlp_step.py, S = 2, with up to 10 000 unlabelled nodes, 500 validation nodes and a validation every 10 steps, three
loops alternated window by window in one process:
  host    what a caller could write before `fit`: per epoch one numpy permutation of the labelled pool, per step one numpy
          permutation of the whole unlabelled pool cut to the batch (what iterate_minibatches_listinputs and sample_unlabel
          draw), `TrainStep.step`; every 10 steps `valid`, two `.item()`s and the early-stop rule in Python, and on an
          improvement a device clone of the state_dict (no file is written, so the comparison is not won on disk I/O)
  fit1    the new loop, the tracker polled at every validation (it stops at the reference's step)
  fit8    the new loop, polled at every 8th validation
Per loop: `<loop>_wall_us` wall clock per step of a window (validations included, the GPU drained at its end) and
`<loop>_host_us`, the host time per step to get the window enqueued; each the median over --reps windows, with the
window-to-window range beside it -- the noise floor of this same-process comparison.  Patience is out of reach, so no
loop stops early.

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
from grand_plus_amd import ClipAdam, Sampler, StepState, TrainStep, valid  # noqa: E402
from grand_plus_amd.fit import FitLoop, early_stop_rule, new_track  # noqa: E402
from grand_plus_amd.mlp import GrandPlusMLP  # noqa: E402
from grand_plus_amd.rows import RowMatrix  # noqa: E402
from grand_plus_amd.step import trained_parameters  # noqa: E402

STEP_CASES = ("cora", "reddit", "amazon2m")
LAM, WARMUP, BASE_SEED, EVAL_BATCH, PATIENCE = 1.0, 100, 0x5EED, 10, 10 ** 9
N_UNLABEL, N_VAL = 10_000, 500
ADAM = dict(lr=1e-2, weight_decay=5e-4, clip_norm=0.1)


def build(name, dev, rng):
    _layout, F, H, C, nl, bn, pin, phid, n_l, n_u, (N, K, kind) = CASES[name]
    S_rows = min(20_000, N)
    seeds = rng.choice(N, S_rows, replace=False).astype(np.int64)
    col, val, filled = synthetic_rows(rng, dev, S_rows, K, N)
    row = torch.from_numpy(np.repeat(seeds, K).astype(np.int32)).to(dev)
    n_train = S_rows // 10
    n_unlabel = min(N_UNLABEL, S_rows - n_train - N_VAL)
    return dict(name=name, rm=RowMatrix(seeds, K, row, col, val, filled, N), X=torch.randn((N, F), device=dev),
                labels=torch.from_numpy(rng.integers(0, C, N)).to(dev), idx_train=seeds[:n_train],
                idx_val=seeds[n_train:n_train + N_VAL], idx_unlabel=seeds[n_train + N_VAL:n_train + N_VAL + n_unlabel],
                batch_size=n_l, unlabel_batch=n_u, kind=kind, model_args=(F, C, H, nl, bn, pin, phid, bn))


def train_step(c, dev):
    torch.manual_seed(0)
    m = GrandPlusMLP(*c["model_args"]).to(dev).train()
    opt = ClipAdam(trained_parameters(m), capturable=True, state=StepState(dev), **ADAM)
    return TrainStep(m, opt, c["rm"], c["X"], c["labels"], c["idx_train"], c["idx_unlabel"], samples=S, dropnode_rate=P_NODE, lam=LAM,
                     warmup=WARMUP, tem=TEM, kind=c["kind"], seed=BASE_SEED, capture=True)


class HostLoop:
    """The loop of before: selections drawn with numpy, every validation read back, the rule and the checkpoint on the host."""

    def __init__(self, c, dev):
        self.c, self.ts = c, train_step(c, dev)
        self.rng = np.random.default_rng(1)
        self.n_train, self.n_unlabel = len(c["idx_train"]), len(c["idx_unlabel"])
        self.t, self.order, self.track, self.saved = 0, None, new_track(), None

    def advance(self):
        c, bs = self.c, self.c["batch_size"]
        nb = -(-self.n_train // bs)
        j = self.t % nb
        if j == 0:
            self.order = self.rng.permutation(self.n_train)                      # once per epoch
        self.t += 1
        unlabel = self.rng.permutation(self.n_unlabel)[:c["unlabel_batch"]]      # the whole pool, every step
        self.ts.step(self.order[j * bs:(j + 1) * bs], unlabel)
        if (self.t - 1) % EVAL_BATCH == 0:
            loss, acc = valid(self.ts.model, c["rm"], c["X"], c["idx_val"], c["labels"], batch_size=bs, dropnode_rate=P_NODE)
            early_stop_rule(self.track, loss.item(), acc.item(), self.t, "both", PATIENCE)
            if self.track["copy_now"]:
                self.saved = {k: v.clone() for k, v in self.ts.model.state_dict().items()}


class FitRun:
    """`fit`'s loop body over a FitLoop that outlives a window."""

    def __init__(self, c, dev, poll_every):
        ts = train_step(c, dev)
        self.loop = FitLoop(ts, Sampler(ts.n_train, ts.n_unlabel, c["batch_size"], c["unlabel_batch"], BASE_SEED), c["idx_val"],
                            eval_batch=EVAL_BATCH, stop_mode="both", patience=PATIENCE)
        self.poll_every = poll_every

    def advance(self):
        loop = self.loop
        if loop.advance() and loop.evals % self.poll_every == 0 and loop.poll().stopped:
            raise RuntimeError("the run stopped early: patience is meant to be out of reach")


def window(run, iters):
    """(wall, host) microseconds per step over one window of `iters` steps."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        run.advance()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6, host / iters * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(STEP_CASES))
    ap.add_argument("--iters", type=int, default=800, help="steps per window (a multiple of 80 polls fit8 evenly)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    for name in a.cases.split(","):
        c = build(name, dev, rng)
        runs = {"host": HostLoop(c, dev), "fit1": FitRun(c, dev, 1), "fit8": FitRun(c, dev, 8)}
        for run in runs.values():                                   # warm-up: code load, every shape's capture, a validation
            for _ in range(2 * -(-len(c["idx_train"]) // c["batch_size"]) + 2 * EVAL_BATCH):
                run.advance()
        torch.cuda.synchronize()
        wall = {k: [] for k in runs}
        host = {k: [] for k in runs}
        for _rep in range(a.reps):
            for k, run in runs.items():                             # alternated: a drift of the clocks reaches all three
                w, h = window(run, a.iters)
                wall[k].append(w)
                host[k].append(h)
        _layout, F, H, C, nl, bn, pin, phid, n_l, n_u, _step = CASES[name]
        rec = {"case": name, "S": S, "batch_size": n_l, "unlabel_batch": n_u, "n_train": len(c["idx_train"]),
               "n_unlabel": len(c["idx_unlabel"]), "n_val": N_VAL, "eval_batch": EVAL_BATCH, "F": F, "H": H, "C": C,
               "iters": a.iters, "reps": a.reps}
        for k in runs:
            rec[k + "_wall_us"] = round(float(np.median(wall[k])), 1)
            rec[k + "_wall_us_range"] = [round(min(wall[k]), 1), round(max(wall[k]), 1)]
            rec[k + "_host_us"] = round(float(np.median(host[k])), 1)
            rec[k + "_host_us_range"] = [round(min(host[k]), 1), round(max(host[k]), 1)]
        for k in ("fit1", "fit8"):
            rec[k + "_speedup_vs_host"] = round(rec["host_wall_us"] / rec[k + "_wall_us"], 2)
        emit(rec, a.out)


if __name__ == "__main__":
    main()
