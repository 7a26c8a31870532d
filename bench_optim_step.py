#!/usr/bin/env python3
"""bench_optim_step.py -- the end of a training step, one JSON line per case.

Not the driver's bench (that is bench.py = GFPush rows/s).  For the parameter tensors of the models of bench_mlp_step.py
(the shapes of run_*.sh), with fixed gradients on every parameter the step trains:
  ours      ClipAdam.step(): one squared-norm launch, one clip + Adam launch
  fused     torch.nn.utils.clip_grad_norm_ + torch.optim.Adam(fused=True).step()
  foreach   torch.nn.utils.clip_grad_norm_ + torch.optim.Adam(foreach=True).step()
The three are alternated in one process: --reps rounds, each timing --iters calls of every variant between CUDA events
(launches and host time included); the median over the rounds is reported, and 28 bytes per element (read p, g, m, v;
write p, m, v) over that time.  --profile-variant <case>:<variant> runs that one variant --iters times with no
warm-up, for a rocprofv3 --kernel-trace --stats run of its own (launches per step = calls / iters).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from _bench_steps import emit, timed  # noqa: E402
from bench_mlp_step import CASES  # noqa: E402
from grand_plus_amd.mlp import GrandPlusMLP, MagMLP  # noqa: E402
from grand_plus_amd.optim import ClipAdam  # noqa: E402

LR, WD, CLIP = 1e-2, 5e-4, 0.1                                      # the run scripts' values


def build(name, dev):
    """Three copies of the case's parameters, each with the same fixed gradients: {variant: step function}, sizes."""
    layout, F, H, C, nl, bn, pin, phid, *_ = CASES[name]
    torch.manual_seed(0)
    cls = GrandPlusMLP if layout == "model" else MagMLP
    model = cls(F if layout == "model" else 1000, C, H, nl, bn, pin, phid, bn).to(dev)
    trained = [(n, p) for n, p in model.named_parameters() if bn or not n.startswith("bns")]   # unused BatchNorms get no gradient
    gen = torch.Generator(device=dev).manual_seed(1)
    grads = [torch.randn(p.shape, generator=gen, device=dev) * 0.01 for _, p in trained]

    def copy():
        ps = [torch.nn.Parameter(p.detach().clone()) for _, p in trained]
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        return ps

    ours_p, fused_p, foreach_p = copy(), copy(), copy()
    ours = ClipAdam(ours_p, lr=LR, weight_decay=WD, clip_norm=CLIP)
    fused = torch.optim.Adam(fused_p, lr=LR, weight_decay=WD, fused=True)
    foreach = torch.optim.Adam(foreach_p, lr=LR, weight_decay=WD, foreach=True)

    def torch_step(opt, ps):
        def go():
            torch.nn.utils.clip_grad_norm_(ps, CLIP)
            opt.step()
        return go

    fns = {"ours": ours.step, "fused": torch_step(fused, fused_p), "foreach": torch_step(foreach, foreach_p)}
    return fns, len(trained), sum(p.numel() for _, p in trained)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--profile-variant", default=None, help="<case>:<variant>: run it --iters times, no warm-up")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    if a.profile_variant:
        name, var = a.profile_variant.split(":")
        fn = build(name, dev)[0][var]
        for _ in range(a.iters):
            fn()
        torch.cuda.synchronize()
        return
    for name in a.cases.split(","):
        fns, n_tensors, n_elems = build(name, dev)
        for fn in fns.values():                                     # warm every variant before the first round
            timed(fn, 10, 1, warmup=10)
        rounds = {k: [] for k in fns}
        for _ in range(a.reps):
            for k, fn in fns.items():
                rounds[k].append(timed(fn, a.iters, 1, warmup=0)[0])
        rec = {"case": name, "tensors": n_tensors, "elements": n_elems, "bytes_per_step": 28 * n_elems, "iters": a.iters,
               "reps": a.reps}
        for k, v in rounds.items():
            rec[k + "_us"] = round(float(np.median(v)), 1)
            rec[k + "_us_range"] = [round(min(v), 1), round(max(v), 1)]
            rec[k + "_gbps"] = round(28 * n_elems / (float(np.median(v)) * 1e-6) / 1e9, 1)
        rec["speedup_vs_fused"] = round(rec["fused_us"] / rec["ours_us"], 2)
        rec["speedup_vs_foreach"] = round(rec["foreach_us"] / rec["ours_us"], 2)
        emit(rec, a.out)


if __name__ == "__main__":
    main()
