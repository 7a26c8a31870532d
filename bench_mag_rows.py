#!/usr/bin/env python3
"""bench_mag_rows.py -- MAG's fused front end against the composed path it replaces, one JSON line per case.

Not the driver's bench (that is bench.py = GFPush rows/s).  Both variants run in one process and alternate window by
window; CUDA events around the whole call, launches and torch's allocations included; median and range of --reps windows
of --iters calls.  Variants:
  fused       mag_prop_rows: one launch forward; torch.zeros + one launch backward
  composed    flatten_rows -> embedding_bag_csr(nodes=nbr) -> random_prop(samples=S, n_out=B), what a step did before (the
              batch changes every step, so flatten_rows and its host read belong to the step); with input dropout the
              embedding is called once per sample, as INTEGRATION §2e had it
  composed_hoisted   the same with flatten_rows taken out of the timed call (bench_mag_step.py's setting)
Cases:
  mag-train        B = 40, K = 32, H = 64, S = 2, forward and backward, input_droprate 0 (run_mag.sh)
  mag-train-pin05  the same at input_droprate 0.5 (bench_mag_step.py's setting)
  mag-valid        B = 100, forward only, eval mode
Every timed call starts from W.grad = None, so a backward is the zero fill, the scatter and nothing else.  The eval-mode
outputs of the two paths are compared once per case (max_abs_diff_eval).  --profile-variant <case>:<variant> runs that one
variant --iters times with no warm-up, for a rocprofv3 --kernel-trace --stats run of its own.

The MAG vocabulary size and bag lengths are not known here: --vocab, --bag and --nodes are the ASSUMPTIONS of
bench_mag_step.py (500 000 attribute ids, 20 attributes per node, 2 000 000 nodes), as are the synthetic [S x K] rows.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from _bench_steps import emit, synthetic_rows, timed  # noqa: E402
from grand_plus_amd.augment import random_prop  # noqa: E402
from grand_plus_amd.embedding import embedding_bag_csr, flatten_rows  # noqa: E402
from grand_plus_amd.mag import mag_prop_rows  # noqa: E402

CASES = {"mag-train": (40, True, 0.0), "mag-train-pin05": (40, True, 0.5), "mag-valid": (100, False, 0.0)}   # B, train, p_in
S, P_NODE = 2, 0.5


def problem(a, dev):
    """The synthetic attribute CSR, table and resident rows every case shares."""
    rng = np.random.default_rng(0)
    N, V, H, K = a.nodes, a.vocab, a.hidden, a.K
    lens = rng.integers(1, 2 * a.bag, N)
    indptr = np.zeros(N + 1, np.int64)
    np.cumsum(lens, out=indptr[1:])
    indices = rng.integers(0, V, int(indptr[-1])).astype(np.int32)
    data = (rng.random(int(indptr[-1]), dtype=np.float32) + 0.05).astype(np.float32)
    ip, ix, dt = (torch.from_numpy(x).to(dev) for x in (indptr, indices, data))
    W = (torch.randn((V, H), device=dev) * 0.1).requires_grad_(True)
    S_rows = 20_000
    col, val, filled = synthetic_rows(rng, dev, S_rows, K, N)
    return rng, ip, ix, dt, W, S_rows, col, val, filled


def build(name, a, prob):
    """The variants of one case as closures over the problem: ({variant: fn}, record fields)."""
    B, train, p_in = CASES[name]
    rng, ip, ix, dt, W, S_rows, col, val, filled = prob
    N, V, H, K = a.nodes, a.vocab, a.hidden, a.K
    dev = W.device
    rows = torch.from_numpy(rng.choice(S_rows, B, replace=False).astype(np.int32)).to(dev)
    hoisted = flatten_rows(col, val, filled, K, rows)

    def composed_from(nbr, scores, mat_idx):
        if not train:
            with torch.no_grad():
                emb = embedding_bag_csr(W, ip, ix, dt, nodes=nbr, training=False, validate=False)
                return random_prop(emb, scores, mat_idx, P_NODE, training=False, n_out=B)
        W.grad = None
        if p_in == 0.0:
            emb = embedding_bag_csr(W, ip, ix, dt, nodes=nbr, input_droprate=0.0, training=True, validate=False)
            loss = random_prop(emb, scores, mat_idx, P_NODE, training=True, samples=S, n_out=B).sum()
        else:
            loss = 0.
            for _ in range(S):                                                   # one embedding per sample
                emb = embedding_bag_csr(W, ip, ix, dt, nodes=nbr, input_droprate=p_in, training=True, validate=False)
                loss = loss + random_prop(emb, scores, mat_idx, P_NODE, training=True, n_out=B).sum()
        loss.backward()

    def fused():
        if not train:
            with torch.no_grad():
                return mag_prop_rows(W, ip, ix, dt, col, val, filled, K, rows, dropnode_rate=P_NODE, training=False)
        W.grad = None
        mag_prop_rows(W, ip, ix, dt, col, val, filled, K, rows, samples=S, dropnode_rate=P_NODE, input_droprate=p_in).sum().backward()

    fns = {"fused": fused, "composed": lambda: composed_from(*flatten_rows(col, val, filled, K, rows)),
           "composed_hoisted": lambda: composed_from(*hoisted)}
    with torch.no_grad():
        e_f = mag_prop_rows(W, ip, ix, dt, col, val, filled, K, rows, training=False)
        emb = embedding_bag_csr(W, ip, ix, dt, nodes=hoisted[0], training=False, validate=False)
        e_c = random_prop(emb, hoisted[1], hoisted[2], P_NODE, training=False, n_out=B)
    nnz = int((ip[hoisted[0] + 1] - ip[hoisted[0]]).sum())
    rec = {"case": name, "B": B, "K": K, "H": H, "S": S if train else 1, "input_droprate": p_in, "backward": train,
           "slots": int(hoisted[0].numel()), "attr_nnz": nnz, "assumed_vocab": V, "assumed_bag_mean": a.bag, "assumed_nodes": N,
           "table_bytes_read": nnz * (4 * H + 8), "max_abs_diff_eval": float((e_f - e_c).abs().max())}
    return fns, rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--nodes", type=int, default=2_000_000)
    ap.add_argument("--vocab", type=int, default=500_000)
    ap.add_argument("--bag", type=int, default=20, help="attributes per node (each node gets 1 .. 2*bag-1, mean bag)")
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--K", type=int, default=32)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--profile-variant", default=None, help="<case>:<variant>: run it --iters times, no warm-up")
    a = ap.parse_args()
    prob = problem(a, torch.device("cuda", 0))
    if a.profile_variant:
        name, var = a.profile_variant.split(":")
        fn = build(name, a, prob)[0][var]
        for _ in range(a.iters):
            fn()
        torch.cuda.synchronize()
        return
    for name in a.cases.split(","):
        fns, rec = build(name, a, prob)
        for fn in fns.values():                                                  # warm every variant before the first round
            timed(fn, 10, 1, warmup=10)
        rounds = {k: [] for k in fns}
        for _ in range(a.reps):
            for k, fn in fns.items():
                rounds[k].append(timed(fn, a.iters, 1, warmup=0)[0])
        rec.update({"iters": a.iters, "reps": a.reps})
        for k, v in rounds.items():
            rec[k + "_us"] = round(float(np.median(v)), 1)
            rec[k + "_us_range"] = [round(min(v), 1), round(max(v), 1)]
        for k in ("composed", "composed_hoisted"):
            rec["speedup_vs_" + k] = round(rec[k + "_us"] / rec["fused_us"], 2)
            spread = (rec["fused_us_range"][1] - rec["fused_us_range"][0]) + (rec[k + "_us_range"][1] - rec[k + "_us_range"][0])
            rec["faster_than_" + k] = bool(rec[k + "_us"] - rec["fused_us"] > spread)     # by more than the two ranges together
        emit(rec, a.out)


if __name__ == "__main__":
    main()
