#!/usr/bin/env python3
"""bench_det_chunk.py -- what `segment_chunk=` does to the deterministic backwards, one JSON line per case.

Not the driver's bench (that is bench.py = GFPush rows/s).  Times the deterministic backward alone -- the sort and index
building, the pre-pass and the gather -- with segment_chunk = None (the unchunked gather_sum_kernel, the yardstick) and
with segment_chunk = 64, 256 and 1024 (gather_chunk_kernel + gather_fold_kernel), the variants alternated window by window
in one process: CUDA events around each window, the median of 5 windows each with [min, max].  The chunked path is never
measured against itself.  Cases, built by bench_det_backward.py's builders:
  mag-train   the embedding bag at the mag-train shape: B = 40 rows, K = 32, H = 64, V = 500 000 uniform ids, mean bag 20
  reddit-rows random_prop_rows at the reddit shape: B = 250, K = 64, F = 602, N = 232 965, --sample 2
  hub-bag     the mag-train shape with one attribute id in every bag
  hub-rows    the reddit shape with node 7 in slot 0 of every row
  zipf-bag    the mag-train shape with attribute ids drawn with probability proportional to 1 / rank over V
and, unless --no-step, the captured MAG step of bench_mag_captured_step.py (replay-det) with Zipf bags, wall clock per step.
Every line carries `longest_segment`, the most sorted positions one destination has in the timed batch; the step's line
takes it over the 64 selections its windows cycle through (`longest_segment_min` is the smallest of them).
No ratio is fixed in advance.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from _bench_steps import emit, timed  # noqa: E402
from bench_det_backward import bag_inputs, rows_inputs  # noqa: E402
from grand_plus_amd import augment, embedding  # noqa: E402

CHUNKS = (None, 64, 256, 1024)


def zipf_ids(V):
    """draw(rng, n): n ids in [0, V), id r - 1 with probability proportional to 1 / r (inverse CDF)."""
    cdf = np.cumsum(1.0 / np.arange(1, V + 1))
    cdf /= cdf[-1]
    return lambda rng, n: np.minimum(np.searchsorted(cdf, rng.random(n)), V - 1)


def key_of(chunk):
    return "unchunked" if chunk is None else f"chunk{chunk}"


def alternate(fns, iters, reps=5, warmup=3):
    """name -> (median, min, max) microseconds per call over `reps` windows each, the variants' windows in turn."""
    for fn in fns.values():
        timed(fn, 1, 1, warmup)
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t[k].append(timed(fn, iters, 1, 0)[0])
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in t.items()}


def longest(sorted_keys, sentinel):
    keys = sorted_keys[sorted_keys != sentinel]
    return int(torch.unique_consecutive(keys, return_counts=True)[1].max()) if keys.numel() else 0


def record(rec, times, out):
    base = times["unchunked"][0]
    for k, (med, lo, hi) in times.items():
        rec[k + "_us"] = round(med, 1)
        rec[k + "_min_max_us"] = [round(lo, 1), round(hi, 1)]
        if k != "unchunked":
            rec[k + "_over_unchunked"] = round(med / base, 3)
    rec["windows"] = 5
    emit(rec, out)


def bag_case(name, dev, rng, V, H, bag, B, K, hub, iters, out, draw_ids=None):
    L, nnz, G, args = bag_inputs(dev, rng, V, H, bag, B, K, hub, draw_ids)
    fns = {key_of(c): (lambda c=c: embedding._backward_det((V, H), G, L, nnz, *args, segment_chunk=c)) for c in CHUNKS}
    times = alternate(fns, iters)
    record({"case": name, "op": "embedding_bag backward, deterministic", "rows": L.nodes.numel(), "attr_nnz": nnz, "H": H,
            "assumed_vocab": V, "assumed_bag_mean": bag, "ids": "zipf" if draw_ids else "uniform", "hub": bool(hub),
            "longest_segment": longest(embedding._det_order(L, nnz, V)[1], V), "iters": iters}, times, out)


def rows_case(name, dev, rng, N, F, B, K, S, hub, iters, out):
    G, args = rows_inputs(dev, rng, N, F, B, K, S, hub)
    col, _, filled, _, rows = args[:5]
    fns = {key_of(c): (lambda c=c: augment._rows_backward_det(G, *args, segment_chunk=c)) for c in CHUNKS}
    times = alternate(fns, iters)
    record({"case": name, "op": "random_prop_rows backward, deterministic", "B": B, "K": K, "F": F, "N": N, "sample": S,
            "hub": bool(hub), "longest_segment": longest(augment._rows_det_order(col, filled, K, rows, N)[1], N), "iters": iters},
           times, out)


def batch_hubs(c, ip, ix, V, K):
    """Per selection the timed windows cycle through: (the entries of its batch, the most entries one attribute id has in
    it), counted as the backward's keys count them: the filled slots of the batch's rows whose column is a node, every
    entry of their bags, ids inside [0, V)."""
    rm = c["rm"]
    pos_all = rm.batch_positions(np.concatenate([c["idx_train"], c["idx_unlabel"]]), check=True).long()
    out = []
    for tr, un in c["sels"]:
        pos = pos_all[torch.from_numpy(np.concatenate([tr, un + c["n_train"]])).to(pos_all.device)]
        cols = rm.col.view(-1, K)[pos].long()
        live = (torch.arange(K, device=cols.device)[None, :] < rm.filled[pos].clamp(0, K)[:, None]) & (cols >= 0) & (cols < rm.n_nodes)
        nodes = cols[live]
        lens = ip[nodes + 1] - ip[nodes]
        first = torch.cumsum(lens, 0) - lens
        where = torch.repeat_interleave(ip[nodes] - first, lens) + torch.arange(int(lens.sum()), device=cols.device)
        ids = ix[where].long()
        ids = ids[(ids >= 0) & (ids < V)]
        out.append((ids.numel(), int(torch.bincount(ids).max()) if ids.numel() else 0))
    return out


def step_case(a, dev, out):
    """bench_mag_captured_step.py's replay-det with Zipf bags, one MagTrainStep per chunk, wall clock per step."""
    import bench_mag_captured_step as cs
    from grand_plus_amd import ClipAdam, MagTrainStep, StepState, mag_trained_parameters
    c = cs.build(a, dev)
    ip, ix, dt = c["attrs"]
    ix = torch.from_numpy(zipf_ids(a.vocab)(np.random.default_rng(1), ix.numel()).astype(np.int32)).to(dev)
    attrs = (ip, ix, dt)
    steps = {}
    for chunk in CHUNKS:
        m = cs.make_model(c, dev)
        ts = MagTrainStep(m, ClipAdam(mag_trained_parameters(m), capturable=True, state=StepState(dev), **cs.ADAM), c["rm"], *attrs,
                          c["labels"], c["idx_train"], c["idx_unlabel"], samples=cs.S, dropnode_rate=cs.P_NODE, lam=cs.LAM,
                          warmup=cs.WARMUP, tem=cs.TEM, kind="l2", seed=cs.BASE_SEED, capture=True, deterministic=True,
                          segment_chunk=chunk)
        steps[key_of(chunk)] = (ts, lambda i, ts=ts: ts.step(*c["sels"][i % cs.N_SELECTIONS]))
    for _, fn in steps.values():
        for i in range(3):
            fn(i)
    torch.cuda.synchronize()
    wall = {k: [] for k in steps}
    for rep in range(a.reps):
        for k, (_, fn) in steps.items():
            wall[k].append(cs.window(fn, a.step_iters, 3 + rep * a.step_iters)[0])
    for ts, _ in steps.values():
        ts.check_entries_flag()
    hubs = batch_hubs(c, ip, ix, a.vocab, a.K)                     # every selection is timed: the windows cycle through them
    ts = steps["unchunked"][0]
    record({"case": "mag-train-step-zipf", "op": "MagTrainStep replay, deterministic", "S": cs.S, "B": cs.N_L + cs.N_U, "K": a.K,
            "H": a.hidden, "assumed_vocab": a.vocab, "assumed_bag_mean": a.bag, "assumed_nodes": a.nodes, "ids": "zipf",
            "max_entries": ts._max_entries(cs.N_L + cs.N_U), "selections": len(hubs),
            "batch_entries_min_max": [min(h[0] for h in hubs), max(h[0] for h in hubs)],
            "longest_segment": max(h[1] for h in hubs), "longest_segment_min": min(h[1] for h in hubs), "iters": a.step_iters},
           {k: (float(np.median(v)), min(v), max(v)) for k, v in wall.items()}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--vocab", type=int, default=500_000)
    ap.add_argument("--bag", type=int, default=20)
    ap.add_argument("--nodes", type=int, default=2_000_000, help="the captured step's node count")
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--K", type=int, default=32)
    ap.add_argument("--step-iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-step", action="store_true", help="leave the captured step out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "det_chunk_bench.jsonl"), help="append the JSON lines to this file too")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    bag_case("mag-train", dev, rng, a.vocab, 64, a.bag, 40, 32, False, a.iters, a.out)
    rows_case("reddit-rows", dev, rng, 232_965, 602, 250, 64, 2, False, a.iters, a.out)
    bag_case("hub-bag", dev, rng, a.vocab, 64, a.bag, 40, 32, True, a.iters, a.out)
    rows_case("hub-rows", dev, rng, 232_965, 602, 250, 64, 2, True, a.iters, a.out)
    bag_case("zipf-bag", dev, rng, a.vocab, 64, a.bag, 40, 32, False, a.iters, a.out, zipf_ids(a.vocab))
    if not a.no_step:
        step_case(a, dev, a.out)


if __name__ == "__main__":
    main()
