#!/usr/bin/env python3
"""bench_infer.py -- the eval pass of get_local_logits, one JSON line per case.

Not the driver's bench (that is bench.py = GFPush rows/s).  Every node's features through the MLP in eval mode, batch
by batch, at the shapes of run_*.sh:
  infer   model.infer(X, out, batch_size): gp_mlp_infer_block per layer and chunk (csrc/mlp_infer.hip)
  block   model.eval(); model(X[chunk]) per chunk, copied into the result: predict's batch loop over the training
          kernels of §7f (csrc/mlp.hip), whose code this benchmark's subject does not change
  torch   model.reference_forward(X[chunk]) under no_grad, copied into the result
The three alternate in one process: one warm-up pass each, then --windows rounds, each timing one whole pass of every
variant between CUDA events (launches and host time included).  Reported: the median and the range of the windows in
ms, TF/s = 2 M sum_l F_l N_l / t, and that over the 155 TF measured peak of the exact-fp32 MFMA.  Before timing, infer's
result is compared with the block path's on the same input.  --profile-variant <case>:<variant> runs one pass of that
variant with no warm-up, for a rocprofv3 --kernel-trace --stats run of its own.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from _bench_steps import emit  # noqa: E402
from grand_plus_amd.mlp import GrandPlusMLP  # noqa: E402

PEAK_TF = 155.0
# name: (rows, F, hidden, classes, layers, BatchNorm + node_norm, batch size)
CASES = {
    "amazon2m_b10000": (2449029, 100, 1024, 47, 2, True, 10000),
    "amazon2m_b100000": (2449029, 100, 1024, 47, 2, True, 100000),
    "reddit": (232965, 602, 512, 41, 2, True, 10000),
    "cora": (2708, 1433, 64, 7, 2, False, 10000),
}


def build(name, dev, rows=None):
    """{variant: one whole pass}, the model, the result buffers and the FLOP of a pass."""
    M, F, H, C, nl, bn, bs = CASES[name]
    M = rows or M
    torch.manual_seed(0)
    model = GrandPlusMLP(F, C, H, nl, bn, 0.0, 0.0, bn).to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(1)
    for b in model.bns:                                              # statistics a trained model would hold
        b.running_mean.copy_(torch.randn(b.running_mean.shape, generator=gen, device=dev) * 0.1)
        b.running_var.copy_(torch.rand(b.running_var.shape, generator=gen, device=dev) + 0.5)
    X = torch.randn((M, F), generator=gen, device=dev)
    outs = {k: torch.empty((M, C), dtype=torch.float32, device=dev) for k in ("infer", "block", "torch")}

    def infer():
        model.infer(X, out=outs["infer"], batch_size=bs)

    def chunks(forward, out):
        def go():
            with torch.no_grad():
                for s in range(0, M, bs):
                    out[s:s + bs].copy_(forward(X[s:s + bs]))
        return go

    fns = {"infer": infer, "block": chunks(model, outs["block"]), "torch": chunks(model.reference_forward, outs["torch"])}
    flop = 2.0 * M * sum(fc.weight.shape[0] * fc.weight.shape[1] for fc in model.fcs)
    return fns, outs, flop, (M, F, H, C, bs)


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--rows", type=int, default=None, help="override the number of rows (a rehearsal at a small size)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--profile-variant", default=None, help="<case>:<variant>: one pass, no warm-up")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    if a.profile_variant:
        name, var = a.profile_variant.split(":")
        build(name, dev, a.rows)[0][var]()
        torch.cuda.synchronize()
        return
    for name in a.cases.split(","):
        fns, outs, flop, (M, F, H, C, bs) = build(name, dev, a.rows)
        for fn in fns.values():                                      # one warm-up pass of every variant
            fn()
        torch.cuda.synchronize()
        diff = float((outs["infer"] - outs["block"]).abs().max())
        scale = float(outs["block"].abs().max())
        ms = {k: [] for k in fns}
        for _ in range(a.windows):
            for k, fn in fns.items():
                ms[k].append(window(fn))
        rec = {"case": name, "rows": M, "shape": [F, H, C], "batch_size": bs, "windows": a.windows, "flop": flop,
               "max_abs_diff_infer_block": diff, "max_abs_block": scale}
        for k, v in ms.items():
            med = float(np.median(v))
            rec[k + "_ms"] = round(med, 3)
            rec[k + "_ms_range"] = [round(min(v), 3), round(max(v), 3)]
            rec[k + "_tflops"] = round(flop / (med * 1e-3) / 1e12, 2)
            rec[k + "_of_peak"] = round(flop / (med * 1e-3) / 1e12 / PEAK_TF, 4)
        noise = (max(ms["infer"]) - min(ms["infer"])) + (max(ms["block"]) - min(ms["block"]))
        rec["speedup_vs_block"] = round(rec["block_ms"] / rec["infer_ms"], 2)
        rec["speedup_vs_torch"] = round(rec["torch_ms"] / rec["infer_ms"], 2)
        rec["faster_than_block_beyond_noise"] = bool(rec["block_ms"] - rec["infer_ms"] > noise)
        emit(rec, a.out)


if __name__ == "__main__":
    main()
