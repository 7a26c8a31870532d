#!/usr/bin/env python3
"""bench_infer_fused.py -- `infer(fused=True)` against `infer` and torch, one JSON line per case.

Not the driver's bench (that is bench.py = GFPush rows/s).  bench_infer.py's method and cases: every node's features
through the MLP in eval mode, batch by batch, at the shapes of run_*.sh:
  infer   model.infer(X, out, batch_size): gp_mlp_infer_block per layer and chunk (csrc/mlp_infer.hip); the yardstick,
          code this benchmark's subject does not change
  fused   model.infer(X, out, batch_size, fused=True): gp_mlp_infer_chain2 per chunk (csrc/mlp_chain.hip)
  torch   model.reference_forward(X[chunk]) under no_grad, copied into the result
The three alternate in one process: one warm-up pass each, then --windows rounds, each timing one whole pass of every
variant between CUDA events (launches and host time included).  Reported: the median and the range of the windows in
ms.  "Faster" is §7j's rule: the fused median lies below the unfused one by more than the two window ranges together.
Before timing, the fused result is compared with the unfused one bit for bit.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from _bench_steps import emit  # noqa: E402
from bench_infer import CASES, window  # noqa: E402
from grand_plus_amd.mlp import GrandPlusMLP  # noqa: E402


def build(name, dev, rows=None):
    """{variant: one whole pass}, the result buffers and the shape."""
    M, F, H, C, nl, bn, bs = CASES[name]
    M = rows or M
    torch.manual_seed(0)
    model = GrandPlusMLP(F, C, H, nl, bn, 0.0, 0.0, bn).to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(1)
    for b in model.bns:                                              # statistics a trained model would hold
        b.running_mean.copy_(torch.randn(b.running_mean.shape, generator=gen, device=dev) * 0.1)
        b.running_var.copy_(torch.rand(b.running_var.shape, generator=gen, device=dev) + 0.5)
    X = torch.randn((M, F), generator=gen, device=dev)
    outs = {k: torch.empty((M, C), dtype=torch.float32, device=dev) for k in ("infer", "fused", "torch")}

    def infer():
        model.infer(X, out=outs["infer"], batch_size=bs)

    def fused():
        model.infer(X, out=outs["fused"], batch_size=bs, fused=True)

    def torch_pass():
        with torch.no_grad():
            for s in range(0, M, bs):
                outs["torch"][s:s + bs].copy_(model.reference_forward(X[s:s + bs]))

    flop = 2.0 * M * sum(fc.weight.shape[0] * fc.weight.shape[1] for fc in model.fcs)
    return {"infer": infer, "fused": fused, "torch": torch_pass}, outs, flop, (M, F, H, C, bs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--rows", type=int, default=None, help="override the number of rows (a rehearsal at a small size)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for name in a.cases.split(","):
        fns, outs, flop, (M, F, H, C, bs) = build(name, dev, a.rows)
        for fn in fns.values():                                      # one warm-up pass of every variant
            fn()
        torch.cuda.synchronize()
        same = bool(torch.equal(outs["fused"].view(torch.int32), outs["infer"].view(torch.int32)))
        ms = {k: [] for k in fns}
        for _ in range(a.windows):
            for k, fn in fns.items():
                ms[k].append(window(fn))
        rec = {"case": name, "rows": M, "shape": [F, H, C], "batch_size": bs, "windows": a.windows, "flop": flop,
               "fused_bits_equal_infer": same}
        for k, v in ms.items():
            med = float(np.median(v))
            rec[k + "_ms"] = round(med, 3)
            rec[k + "_ms_range"] = [round(min(v), 3), round(max(v), 3)]
            rec[k + "_tflops"] = round(flop / (med * 1e-3) / 1e12, 2)
        noise = (max(ms["fused"]) - min(ms["fused"])) + (max(ms["infer"]) - min(ms["infer"]))
        noise_t = (max(ms["fused"]) - min(ms["fused"])) + (max(ms["torch"]) - min(ms["torch"]))
        rec["speedup_vs_infer"] = round(rec["infer_ms"] / rec["fused_ms"], 2)
        rec["speedup_vs_torch"] = round(rec["torch_ms"] / rec["fused_ms"], 2)
        rec["faster_than_infer_beyond_noise"] = bool(rec["infer_ms"] - rec["fused_ms"] > noise)
        rec["faster_than_torch_beyond_noise"] = bool(rec["torch_ms"] - rec["fused_ms"] > noise_t)
        emit(rec, a.out)


if __name__ == "__main__":
    main()
