#!/usr/bin/env python3
"""bench_train_step.py -- the per-step math of GRAND+ training after the precompute, one JSON line per case.

Not the driver's bench (that is bench.py = GFPush rows/s).  At the training shapes of run_*.sh (--sample 2), per case:
  objective     logits z [S, B, C] (a leaf) -> loss -> backward
                ours: grand_plus_loss (one forward, one reduce, one backward launch, no host synchronisation)
                reference formulation: log_softmax + F.nll_loss per sample + consis_loss (model.py:123-139, 321-331)
  aug_objective S augmentations -> a linear head per sample (the same torch matmul on both sides, standing in for
                the MLP, which stays PyTorch) -> the objective -> backward
                ours: random_prop_rows(samples=S) from the resident [S_rows x K] rows (MAG: the COO form with n_out
                and a feature operand that takes a gradient, as MAG's embedding output does)
                reference formulation: S x random_prop as index_add_ on device COO tensors (torch_scatter's
                semantics) + the objective above
Times are CUDA events around the whole step (launches included), median of --reps windows of --iters steps.
--profile-variant runs one variant of one case for --iters steps with no warm-up, for a rocprofv3 --kernel-trace
--stats run of its own (launches per step = calls / iters).

Graphs, features and rows are synthetic (node counts of the datasets, uniform random neighbours and scores).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from _bench_steps import batch_of, emit, synthetic_rows, timed, torch_prop  # noqa: E402
from grand_plus_amd.augment import random_prop, random_prop_rows  # noqa: E402
from grand_plus_amd.objective import grand_plus_loss  # noqa: E402
from oracle.objective_ref import grand_loss_ref  # noqa: E402

# name: nodes, F (MAG: H), C, labelled, unlabelled, K, loss kind  (run_*.sh; tem 0.1 everywhere, --sample 2)
CASES = {
    "reddit": (232_965, 602, 41, 50, 200, 64, "kl"),
    "amazon2m": (2_449_029, 100, 47, 50, 200, 64, "kl"),
    "cora": (2_708, 1433, 7, 50, 100, 32, "l2"),
    "mag": (None, 64, 8, 20, 20, 32, "l2"),
}
S, TEM, P_NODE = 2, 0.1, 0.5


def build(name, dev, rng):
    N, F, C, n_l, n_u, K, kind = CASES[name]
    B = n_l + n_u
    S_rows = 20_000
    n_nodes = N if N is not None else S_rows * K
    col, val, filled = synthetic_rows(rng, dev, S_rows, K, n_nodes)
    rows, nbr, scores, idx = batch_of(rng, dev, col, val, S_rows, K, B)
    labels = torch.from_numpy(rng.integers(0, C, n_l)).to(dev)
    head = (torch.randn((F, C), device=dev) * 0.05).requires_grad_(True)
    if N is None:                                                   # MAG: the embedding output of the batch, trained
        X = None
        feats = (torch.randn((B * K, F), device=dev) * 0.1).requires_grad_(True)
    else:
        X = torch.randn((N, F), device=dev)
        feats = X[nbr]
    return dict(N=N, F=F, C=C, n_l=n_l, B=B, K=K, kind=kind, col=col, val=val, filled=filled, rows=rows, labels=labels,
                head=head, X=X, feats=feats, scores=scores, idx=idx)


def variants(c):
    n_l, B, C, kind, K, head = c["n_l"], c["B"], c["C"], c["kind"], c["K"], c["head"]
    z_ours = torch.randn((S, B, C), device=head.device).mul_(3).requires_grad_(True)
    z_ref = [z_ours[s].detach().clone().requires_grad_(True) for s in range(S)]

    def ours_objective():
        loss, _ = grand_plus_loss(z_ours, c["labels"], n_l, 1.0, tem=TEM, kind=kind)
        loss.backward()

    def ref_objective_only():
        grand_loss_ref(z_ref, c["labels"], n_l, 1.0, TEM, 2.0 / C, kind)[0].backward()

    def ours_step():
        if c["X"] is not None:
            aug = random_prop_rows(c["X"], c["col"], c["val"], c["filled"], K, batch_rows=c["rows"], dropnode_rate=P_NODE,
                                   training=True, samples=S)
        else:
            aug = random_prop(c["feats"], c["scores"], c["idx"], P_NODE, training=True, samples=S, n_out=B)
        loss, _ = grand_plus_loss([aug[s] @ head for s in range(S)], c["labels"], n_l, 1.0, tem=TEM, kind=kind)
        loss.backward()

    def ref_step():
        logits = [torch_prop(c["feats"], c["scores"], c["idx"], P_NODE, True, B) @ head for _ in range(S)]
        grand_loss_ref(logits, c["labels"], n_l, 1.0, TEM, 2.0 / C, kind)[0].backward()

    return {"ours_objective": ours_objective, "ref_objective": ref_objective_only, "ours_step": ours_step, "ref_step": ref_step}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="reddit,amazon2m,cora,mag")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--profile-variant", default=None, help="run one variant of the first case for --iters steps, no warm-up")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    if a.profile_variant:
        c = build(a.cases.split(",")[0], dev, rng)
        fn = variants(c)[a.profile_variant]
        for _ in range(a.iters):
            fn()
        torch.cuda.synchronize()
        return
    for name in a.cases.split(","):
        c = build(name, dev, rng)
        v = variants(c)
        rec = {"case": name, "S": S, "B": c["B"], "labelled": c["n_l"], "K": c["K"], "F": c["F"], "C": c["C"], "loss": c["kind"],
               "tem": TEM, "iters": a.iters, "reps": a.reps}
        for key in ("ours_objective", "ref_objective", "ours_step", "ref_step"):
            med, lo, hi = timed(v[key], a.iters, a.reps, warmup=5)
            rec[key + "_us"] = round(med, 1)
            rec[key + "_us_range"] = [round(lo, 1), round(hi, 1)]
        rec["objective_speedup"] = round(rec["ref_objective_us"] / rec["ours_objective_us"], 2)
        rec["step_speedup"] = round(rec["ref_step_us"] / rec["ours_step_us"], 2)
        emit(rec, a.out)


if __name__ == "__main__":
    main()
