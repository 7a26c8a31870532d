#!/usr/bin/env python3
"""bench_dense.py -- what the dense-LDS GFPush kernel (option kernel = 3) does on the graphs it is for, one JSON
line per graph, recipe and variant.

Not the driver's bench (that is bench.py; `bench.py --workload cora --opt kernel=3` gives the driver-style line).  Times
gfpush_device alone on the Cora and Citeseer CSRs and recipes of tests/golden/*.npz, seeds cycled to 16 384 rows, under
  kernel1        option kernel = 1: the general kernel, the yardstick
  dense          option kernel = 3, dn_csr_lds = 0: the CSR read from memory (it lives in L2)
  dense-csr-lds  option kernel = 3, dn_csr_lds = 1: indptr + indices staged into LDS once per workgroup
the variants alternated window by window in one process: CUDA events around each window, the median of 5 windows each with
[min, max].  --blocks adds dense variants at other workgroup sizes (dn_block_threads).  Every line carries rows_per_s and its
ratio over kernel1 of the same graph and recipe.  No ratio is fixed in advance.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from _bench_steps import emit, timed  # noqa: E402
from grand_plus_amd import Graph  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def alternate(fns, iters, reps=5, warmup=2):
    """name -> (median, min, max) microseconds per call over `reps` windows each, the variants' windows in turn."""
    for fn in fns.values():
        timed(fn, 1, 1, warmup)
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t[k].append(timed(fn, iters, 1, 0)[0])
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in t.items()}


def variants(blocks):
    out = {"kernel1": {"kernel": 1}}
    for b in blocks:
        tag = "" if b == 0 else f"-x{b}"
        extra = {} if b == 0 else {"dn_block_threads": b}
        out["dense" + tag] = dict(extra, kernel=3, dn_csr_lds=0)
        out["dense-csr-lds" + tag] = dict(extra, kernel=3, dn_csr_lds=1)
    return out


def case(name, mode, rows, iters, blocks, dev, out):
    z = np.load(os.path.join(GOLD, f"{name}.npz"))
    coef, rmax, K = z[f"{mode}_coef"], float(z[f"{mode}_params"][0]), int(z[f"{mode}_params"][1])
    seeds = torch.from_numpy(np.resize(z["seeds"].astype(np.int32), rows)).to(dev)
    bufs = (torch.zeros(rows * K, dtype=torch.int32, device=dev), torch.zeros(rows * K, dtype=torch.int32, device=dev),
            torch.zeros(rows * K, dtype=torch.float64, device=dev), torch.zeros(rows, dtype=torch.int32, device=dev))
    graphs, fns = {}, {}
    for key, opts in variants(blocks).items():
        g = Graph(z["indptr"], z["indices"], 0)
        for k, v in opts.items():
            g.set_option(k, v)
        graphs[key] = g
        fns[key] = lambda g=g: g.gfpush_device(seeds, coef, rmax, K, *bufs)
    times = alternate(fns, iters)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    base = times["kernel1"][0]
    for key, (med, lo, hi) in times.items():
        st = graphs[key].stats()
        emit({"graph": name, "mode": mode, "variant": key, "kernel": st["kernel"], "rows": rows, "K": K, "rmax": rmax, "n_coef": len(coef),
              "block_threads": st["block_threads"], "lds_bytes": st["lds_bytes"], "workgroups": st["workgroups"],
              "workgroups_per_cu": round(st["workgroups"] / cus, 2), "us_per_call": round(med, 1), "min_max_us": [round(lo, 1), round(hi, 1)],
              "rows_per_s": round(rows / med * 1e6), "over_kernel1": round(base / med, 3), "windows": 5, "iters": iters}, out)
    for g in graphs.values():
        g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--iters", type=int, default=3, help="calls per window")
    ap.add_argument("--blocks", default="0", help="comma-separated dn_block_threads of the dense variants (0 = the default)")
    ap.add_argument("--graphs", default="cora,citeseer")
    ap.add_argument("--modes", default="ppr,avg,single")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_bench.jsonl"), help="append the JSON lines to this file too")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for name in a.graphs.split(","):
        for mode in a.modes.split(","):
            case(name, mode, a.rows, a.iters, [int(b) for b in a.blocks.split(",")], dev, a.out)


if __name__ == "__main__":
    main()
