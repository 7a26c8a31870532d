#!/usr/bin/env python3
"""bench_valid.py -- the validation pass of `fit` batched, in one pass and captured, one JSON line per case.

Not the driver's bench (that is bench.py = GFPush rows/s).  bench_fit.py's three step shapes and its window scheme: the
loops alternated window by window in one process, the median over --reps windows with the window-to-window [min, max]
beside it.  Four `fit` loops, the tracker polled at every validation (bench_fit.py's fit1):
  fit1       `fit` as it is: the validation in batches of the training batch size, every launch issued from Python
  capture    valid_capture=True alone: the same batches, replayed from one captured graph with the tracker's update
  one_pass   valid_one_pass=True alone: one gather, one `infer`, one `eval_tail`, issued from Python
  both       the one pass, replayed
`<loop>_wall_us` is the wall clock per step of a window (validations included, the GPU drained at its end) and
`<loop>_host_us` the host time per step to get the window enqueued.  A variant "pays" only where its window range lies
wholly below fit1's.

Then one validation pass on its own, wall microseconds per pass over --pass-iters back-to-back passes (drained at the end),
in the same four forms (`pass_*_us`), and the evaluation tail alone over the pass's 500 logit rows, `eval_tail` against
`eval_head` + `eval_reduce`, issued eagerly and replayed from a graph of 20 calls (`tail_*_us`, per call).

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

from _bench_steps import emit  # noqa: E402
from bench_fit import BASE_SEED, EVAL_BATCH, N_VAL, PATIENCE, STEP_CASES, build, train_step, window  # noqa: E402
from bench_mlp_step import CASES, P_NODE, S  # noqa: E402
from grand_plus_amd import Sampler, eval_head, eval_reduce, eval_tail  # noqa: E402
from grand_plus_amd.evaluate import ValidGraph, eval_buffers, eval_tail_workspace, valid_pass  # noqa: E402
from grand_plus_amd.fit import FitLoop  # noqa: E402

LOOPS = {"fit1": {}, "capture": dict(valid_capture=True), "one_pass": dict(valid_one_pass=True),
         "both": dict(valid_one_pass=True, valid_capture=True)}
GRAPH_CALLS = 20


class FitRun:
    """`fit`'s loop body over a FitLoop that outlives a window, polled at every validation."""

    def __init__(self, c, dev, **kw):
        self.ts = train_step(c, dev)
        self.loop = FitLoop(self.ts, Sampler(self.ts.n_train, self.ts.n_unlabel, c["batch_size"], c["unlabel_batch"], BASE_SEED),
                            c["idx_val"], eval_batch=EVAL_BATCH, stop_mode="both", patience=PATIENCE, **kw)

    def advance(self):
        loop = self.loop
        if loop.advance() and loop.poll().stopped:
            raise RuntimeError("the run stopped early: patience is meant to be out of reach")


def per_call(fn, iters, reps):
    """[wall microseconds per call] over reps windows of iters back-to-back calls, the GPU drained at each window's end."""
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / iters * 1e6)
    return out


def put(rec, key, samples):
    rec[key] = round(float(np.median(samples)), 2)
    rec[key + "_range"] = [round(min(samples), 2), round(max(samples), 2)]


def graph_of(body):
    body()                                                   # eager first: code load
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(GRAPH_CALLS):
            body()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(STEP_CASES))
    ap.add_argument("--iters", type=int, default=800, help="steps per window")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pass-iters", type=int, default=200, help="validation passes (tail calls: ten times as many) per window")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    for name in a.cases.split(","):
        c = build(name, dev, rng)
        runs = {k: FitRun(c, dev, **kw) for k, kw in LOOPS.items()}
        for run in runs.values():                                   # warm-up: code load, every shape's capture, three validations
            for _ in range(2 * -(-len(c["idx_train"]) // c["batch_size"]) + 3 * EVAL_BATCH):
                run.advance()
        torch.cuda.synchronize()
        wall = {k: [] for k in runs}
        host = {k: [] for k in runs}
        for _rep in range(a.reps):
            for k, run in runs.items():                             # alternated: a drift of the clocks reaches all four
                w, h = window(run, a.iters)
                wall[k].append(w)
                host[k].append(h)
        _layout, F, H, C, nl, bn, pin, phid, n_l, n_u, _step = CASES[name]
        rec = {"case": name, "S": S, "batch_size": n_l, "unlabel_batch": n_u, "n_val": N_VAL, "eval_batch": EVAL_BATCH, "F": F, "H": H,
               "C": C, "iters": a.iters, "reps": a.reps, "pass_iters": a.pass_iters}
        for k in runs:
            put(rec, k + "_wall_us", wall[k])
            put(rec, k + "_host_us", host[k])
        for k in ("capture", "one_pass", "both"):
            rec[k + "_pays"] = bool(max(wall[k]) < min(wall["fit1"]))
            rec[k + "_vs_fit1"] = round(rec["fit1_wall_us"] / rec[k + "_wall_us"], 3)

        # one validation pass on its own, in the four forms (the graphs carry no tracker: the pass alone)
        ts = runs["fit1"].ts
        batched, one = ts._valid_plan(c["idx_val"], n_l), ts._valid_plan(c["idx_val"], n_l, one_pass=True)
        forms = {"pass_batched_eager": lambda: valid_pass(batched, P_NODE), "pass_one_eager": lambda: valid_pass(one, P_NODE)}
        for key, plan in (("pass_batched_replay", batched), ("pass_one_replay", one)):
            vg = ValidGraph(plan, P_NODE)
            vg.run()
            vg.run()                                                # the capture
            forms[key] = vg.run
        for fn in forms.values():
            fn()
        samples = {k: [] for k in forms}
        for _rep in range(a.reps):
            for k, fn in forms.items():
                samples[k] += per_call(fn, a.pass_iters, 1)
        for k in forms:
            put(rec, k + "_us", samples[k])

        # the tail alone over the pass's logits
        z = torch.randn((N_VAL, C), device=dev)
        idx = one.idx
        buf, ws = eval_buffers(N_VAL, dev), eval_tail_workspace(dev)
        res = (torch.empty(2, device=dev), torch.empty(4, dtype=torch.int64, device=dev))

        def fused():
            eval_tail(z, c["labels"], label_rows=idx, out=buf, workspace=ws, result=res)

        def pair():
            eval_reduce(eval_head(z, c["labels"], label_rows=idx, out=buf))

        gf, gp = graph_of(fused), graph_of(pair)
        tails = {"tail_fused_eager": (fused, 1), "tail_pair_eager": (pair, 1), "tail_fused_replay": (gf.replay, GRAPH_CALLS),
                 "tail_pair_replay": (gp.replay, GRAPH_CALLS)}
        samples = {k: [] for k in tails}
        for _rep in range(a.reps):
            for k, (fn, calls) in tails.items():
                samples[k] += [x / calls for x in per_call(fn, a.pass_iters * 10 // calls, 1)]
        for k in tails:
            put(rec, k + "_us", samples[k])
        emit(rec, a.out)


if __name__ == "__main__":
    main()
