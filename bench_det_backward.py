#!/usr/bin/env python3
"""bench_det_backward.py -- what the deterministic backwards cost, one JSON line per case.

Not the driver's bench (that is bench.py = GFPush rows/s).  Times the backward alone -- the gradient kernel(s) and, for the
deterministic path, the sort and index building in front of them -- of the atomic path (the default; the parent commit's
kernel) against the deterministic one, in alternating windows of one process: CUDA events around each window, the median
of 5 windows each (_bench_steps.timed's loop, one window per call so that the two paths alternate).  Cases:
  mag-train   the embedding bag at the mag-train shape: B = 40 rows, K = 32, H = 64, --sample 2 (two backwards per step),
              V = 500 000 attribute ids, mean bag 20 (ASSUMPTIONS, as in bench_mag_step.py)
  reddit-rows random_prop_rows at the reddit shape: B = 250, K = 64, F = 602, N = 232 965, --sample 2
  hub-bag     the mag-train shape with one attribute id in every bag (a serial chain of adds on one wave)
  hub-rows    the reddit shape with node 7 in slot 0 of every row
No ratio is fixed in advance: the deterministic path sorts and is expected to be slower.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from _bench_steps import emit, synthetic_rows, timed  # noqa: E402
from grand_plus_amd import augment, embedding  # noqa: E402


def alternate(atomic, det, iters, reps=5, warmup=3):
    """Median microseconds per call of the two paths over `reps` windows each, atomic and deterministic windows in turn."""
    timed(atomic, 1, 1, warmup)
    timed(det, 1, 1, warmup)
    a, d = [], []
    for _ in range(reps):
        a.append(timed(atomic, iters, 1, 0)[0])
        d.append(timed(det, iters, 1, 0)[0])
    return float(np.median(a)), float(np.median(d)), (min(a), max(a)), (min(d), max(d))


def bag_inputs(dev, rng, V, H, bag, B, K, hub, draw_ids=None):
    """The embedding bag's backward operands at one shape: (L, nnz, G, args) for embedding._backward / _backward_det.
    draw_ids(rng, n): the attribute ids of the n stored entries (default: uniform over V); bench_det_chunk.py builds its
    cases here too."""
    n_nodes = 200_000
    lens = rng.integers(1, 2 * bag, n_nodes)
    indptr = np.zeros(n_nodes + 1, np.int64); np.cumsum(lens, out=indptr[1:])
    n_stored = int(indptr[-1])
    indices = (rng.integers(0, V, n_stored) if draw_ids is None else draw_ids(rng, n_stored)).astype(np.int32)
    if hub:
        indices[indptr[:-1]] = 13                                               # the first attribute of every node
    data = (rng.random(n_stored, dtype=np.float32) + 0.05).astype(np.float32)
    ip, ix, dt = (torch.from_numpy(x).to(dev) for x in (indptr, indices, data))
    nodes = torch.from_numpy(rng.integers(0, n_nodes, B * K)).to(dev)            # the batch's B * K neighbour rows
    bl = ip[nodes + 1] - ip[nodes]
    L = embedding._Layout(ip, n_nodes, nodes, torch.cumsum(bl, 0) - bl, nodes.numel(), ix, dt)
    nnz = int(bl.sum())
    G = torch.randn((nodes.numel(), H), device=dev)
    return L, nnz, G, (0.5, True, 1234, None)


def bag_case(name, dev, rng, V, H, bag, B, K, hub, iters, out):
    L, nnz, G, args = bag_inputs(dev, rng, V, H, bag, B, K, hub)
    nodes = L.nodes
    atomic = lambda: embedding._backward((V, H), G, L, *args)                    # noqa: E731
    det = lambda: embedding._backward_det((V, H), G, L, nnz, *args)              # noqa: E731
    a, d, ar, dr = alternate(atomic, det, iters)
    sort_only = timed(lambda: embedding._det_order(L, nnz, V), iters, 5, 3)[0]
    zero_only = timed(lambda: torch.zeros((V, H), device=dev), iters, 5, 3)[0]
    emit({"case": name, "op": "embedding_bag backward", "rows": nodes.numel(), "attr_nnz": nnz, "H": H, "assumed_vocab": V,
          "assumed_bag_mean": bag, "hub": bool(hub), "atomic_us": round(a, 1), "deterministic_us": round(d, 1),
          "det_over_atomic": round(d / a, 2), "atomic_min_max_us": [round(x, 1) for x in ar],
          "deterministic_min_max_us": [round(x, 1) for x in dr], "sort_and_index_us": round(sort_only, 1),
          "zeroing_dW_us": round(zero_only, 1), "windows": 5, "iters": iters}, out)


def rows_inputs(dev, rng, N, F, B, K, S, hub):
    """random_prop_rows' backward operands at one shape: (G, args) for augment._rows_backward / _rows_backward_det."""
    S_rows = 20_000
    col, val, filled = synthetic_rows(rng, dev, S_rows, K, N)
    if hub:
        col.view(S_rows, K)[:, 0] = 7
    rows = torch.from_numpy(rng.choice(S_rows, B, replace=False).astype(np.int32)).to(dev)
    G = torch.randn((S, B, F), device=dev)
    return G, (col, val, filled, K, rows, B, N, S, 0.5, True, 99, None)


def rows_case(name, dev, rng, N, F, B, K, S, hub, iters, out):
    G, args = rows_inputs(dev, rng, N, F, B, K, S, hub)
    col, _, filled, _, rows = args[:5]
    atomic = lambda: augment._rows_backward(G, *args)                            # noqa: E731
    det = lambda: augment._rows_backward_det(G, *args)                           # noqa: E731
    a, d, ar, dr = alternate(atomic, det, iters)
    sort_only = timed(lambda: augment._rows_det_order(col, filled, K, rows, N), iters, 5, 3)[0]
    zero_only = timed(lambda: torch.zeros((N, F), device=dev), iters, 5, 3)[0]
    emit({"case": name, "op": "random_prop_rows backward", "B": B, "K": K, "F": F, "N": N, "sample": S, "hub": bool(hub),
          "atomic_us": round(a, 1), "deterministic_us": round(d, 1), "det_over_atomic": round(d / a, 2),
          "atomic_min_max_us": [round(x, 1) for x in ar], "deterministic_min_max_us": [round(x, 1) for x in dr],
          "sort_and_index_us": round(sort_only, 1), "zeroing_grad_us": round(zero_only, 1), "windows": 5, "iters": iters}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--vocab", type=int, default=500_000)
    ap.add_argument("--bag", type=int, default=20)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    bag_case("mag-train", dev, rng, a.vocab, 64, a.bag, 40, 32, False, a.iters, a.out)
    rows_case("reddit-rows", dev, rng, 232_965, 602, 250, 64, 2, False, a.iters, a.out)
    bag_case("hub-bag", dev, rng, a.vocab, 64, a.bag, 40, 32, True, a.iters, a.out)
    rows_case("hub-rows", dev, rng, 232_965, 602, 250, 64, 2, True, a.iters, a.out)


if __name__ == "__main__":
    main()
