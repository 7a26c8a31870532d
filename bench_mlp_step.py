#!/usr/bin/env python3
"""bench_mlp_step.py -- GRAND+'s MLP in a training step, one JSON line per case.

Not the driver's bench (that is bench.py = GFPush rows/s).  At the shapes of run_*.sh, --sample 2:
  mlp           x [S, B, F] (no grad, as random_prop's output is detached in model.py:322) -> MLP -> backward(dy)
                ours:  GrandPlusMLP, all S samples per layer in one set of HIP launches
                torch: the same module's torch path (reference_forward), called S times as model.py:321-325 does
  step          (cases with a training step in bench_train_step.py) -> loss -> backward, three ways
                ours:  random_prop_rows(samples=2) -> GrandPlusMLP -> grand_plus_loss (MAG: the COO form, MagMLP)
                s7e:   random_prop_rows(samples=2) -> the torch MLP per sample -> grand_plus_loss (DESIGN §7e's step)
                ref:   S x random_prop as index_add_ -> the torch MLP -> log_softmax + nll_loss + consis_loss
  eval          (--eval) get_local_logits at the Amazon2M shape: the eval-mode MLP over 2 449 029 rows in batches of
                --eval-batch rows, ours against the torch path
Times are CUDA events around the whole call (launches included), median of --reps windows of --iters calls.
--profile-variant <case>:<variant> runs that one variant for --iters calls with no warm-up, for a rocprofv3
--kernel-trace --stats run of its own (launches per step = calls / iters).

Features, graphs and rows are synthetic (uniform random neighbours and scores).
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
from grand_plus_amd.mlp import GrandPlusMLP, MagMLP  # noqa: E402
from grand_plus_amd.objective import grand_plus_loss  # noqa: E402
from oracle.objective_ref import grand_loss_ref  # noqa: E402

# name: layout, F, H, C, nlayers, use_bn/node_norm, input/hidden dropout, labelled + unlabelled rows, step (nodes, K, loss)
CASES = {
    "cora": ("model", 1433, 64, 7, 2, False, 0.5, 0.7, 50, 100, (2_708, 32, "l2")),
    "citeseer": ("model", 3703, 256, 6, 2, False, 0.0, 0.0, 50, 200, None),
    "pubmed": ("model", 500, 32, 3, 1, True, 0.2, 0.2, 50, 200, None),
    "reddit": ("model", 602, 512, 41, 2, True, 0.0, 0.0, 50, 200, (232_965, 64, "kl")),
    "amazon2m": ("model", 100, 1024, 47, 2, True, 0.0, 0.0, 50, 200, (2_449_029, 64, "kl")),
    "aminer": ("model", 100, 32, 18, 1, True, 0.0, 0.0, 50, 200, None),
    "mag": ("mag", 64, 64, 8, 2, False, 0.0, 0.2, 20, 20, (None, 32, "l2")),
}
S, TEM, P_NODE = 2, 0.1, 0.5
AMAZON2M_NODES = 2_449_029


def build(name, dev, rng):
    layout, F, H, C, nl, bn, pin, phid, n_l, n_u, step = CASES[name]
    B = n_l + n_u
    torch.manual_seed(0)
    cls = GrandPlusMLP if layout == "model" else MagMLP
    model = cls(F if layout == "model" else 1000, C, H, nl, bn, pin, phid, bn).to(dev).train()
    Fin = F if layout == "model" else H
    c = dict(name=name, model=model, B=B, n_l=n_l, C=C, F=Fin, H=H, layout=layout,
             x=torch.randn((S, B, Fin), device=dev), dy=torch.randn((S, B, C), device=dev) * 0.01,
             labels=torch.from_numpy(rng.integers(0, C, n_l)).to(dev))
    if step is not None:
        N, K, kind = step
        S_rows = 20_000
        n_nodes = N if N is not None else S_rows * K
        col, val, filled = synthetic_rows(rng, dev, S_rows, K, n_nodes)
        rows, nbr, scores, idx = batch_of(rng, dev, col, val, S_rows, K, B)
        c.update(K=K, kind=kind, col=col, val=val, rows=rows, filled=filled, nbr=nbr, scores=scores, idx=idx)
        if N is None:                                               # MAG: the embedding output of the batch, trained
            c["X"] = None
            c["feats"] = (torch.randn((B * K, Fin), device=dev) * 0.1).requires_grad_(True)
        else:
            c["X"] = torch.randn((N, Fin), device=dev)
            c["feats"] = c["X"][c["nbr"]]
    return c


def variants(c):
    m, x, dy, B, n_l, C = c["model"], c["x"], c["dy"], c["B"], c["n_l"], c["C"]

    def mlp_ours():
        m(x).backward(dy)

    def mlp_torch():
        outs = [m.reference_forward(x[s]) for s in range(S)]
        torch.autograd.backward(outs, [dy[s] for s in range(S)])

    v = {"mlp_ours": mlp_ours, "mlp_torch": mlp_torch}
    if "K" not in c:
        return v
    K, kind = c["K"], c["kind"]

    def aug():
        if c["X"] is not None:
            return random_prop_rows(c["X"], c["col"], c["val"], c["filled"], K, batch_rows=c["rows"], dropnode_rate=P_NODE,
                                    training=True, samples=S)
        return random_prop(c["feats"], c["scores"], c["idx"], P_NODE, training=True, samples=S, n_out=B)

    def step_ours():
        loss, _ = grand_plus_loss(m(aug()), c["labels"], n_l, 1.0, tem=TEM, kind=kind)
        loss.backward()

    def step_s7e():
        a = aug()
        loss, _ = grand_plus_loss([m.reference_forward(a[s]) for s in range(S)], c["labels"], n_l, 1.0, tem=TEM, kind=kind)
        loss.backward()

    def step_ref():
        logits = [m.reference_forward(torch_prop(c["feats"], c["scores"], c["idx"], P_NODE, True, B)) for _ in range(S)]
        grand_loss_ref(logits, c["labels"], n_l, 1.0, TEM, 2.0 / C, kind)[0].backward()

    v.update(step_ours=step_ours, step_s7e=step_s7e, step_ref=step_ref)
    return v


def eval_variants(dev, batch):
    layout, F, H, C, nl, bn, pin, phid, *_ = CASES["amazon2m"]
    torch.manual_seed(0)
    m = GrandPlusMLP(F, C, H, nl, bn, pin, phid, bn).to(dev).eval()
    X = torch.randn((AMAZON2M_NODES, F), device=dev)
    out = torch.empty((AMAZON2M_NODES, C), device=dev)

    def run(fn):
        def go():
            with torch.no_grad():
                for i in range(0, AMAZON2M_NODES, batch):
                    out[i:i + batch] = fn(X[i:i + batch])
        return go

    return {"eval_ours": run(m), "eval_torch": run(m.reference_forward)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--eval", action="store_true", help="also time get_local_logits at the Amazon2M shape")
    ap.add_argument("--eval-batch", type=int, default=10_000)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--profile-variant", default=None, help="<case>:<variant>: run it --iters times, no warm-up")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    if a.profile_variant:
        name, var = a.profile_variant.split(":")
        fn = eval_variants(dev, a.eval_batch)[var] if name == "eval" else variants(build(name, dev, rng))[var]
        for _ in range(a.iters):
            fn()
        torch.cuda.synchronize()
        return
    for name in a.cases.split(","):
        c = build(name, dev, rng)
        layout, F, H, C, nl, bn, pin, phid, n_l, n_u, _ = CASES[name]
        rec = {"case": name, "layout": layout, "S": S, "B": c["B"], "F": F, "H": H, "C": C, "nlayers": nl, "bn_norm": bn,
               "dropout": [pin, phid], "iters": a.iters, "reps": a.reps}
        for key, fn in variants(c).items():
            med, lo, hi = timed(fn, a.iters, a.reps, warmup=3)
            rec[key + "_us"] = round(med, 1)
            rec[key + "_us_range"] = [round(lo, 1), round(hi, 1)]
        rec["mlp_speedup"] = round(rec["mlp_torch_us"] / rec["mlp_ours_us"], 2)
        if "step_ours_us" in rec:
            rec["step_speedup_vs_s7e"] = round(rec["step_s7e_us"] / rec["step_ours_us"], 2)
            rec["step_speedup_vs_ref"] = round(rec["step_ref_us"] / rec["step_ours_us"], 2)
            rec["mlp_share_of_s7e_step"] = round(rec["mlp_torch_us"] / rec["step_s7e_us"], 2)
        emit(rec, a.out)
    if a.eval:
        rec = {"case": "amazon2m_get_local_logits", "rows": AMAZON2M_NODES, "batch": a.eval_batch, "iters": 1, "reps": 3}
        for key, fn in eval_variants(dev, a.eval_batch).items():
            med, lo, hi = timed(fn, 1, 3, warmup=3)
            rec[key + "_us"] = round(med, 1)
            rec[key + "_us_range"] = [round(lo, 1), round(hi, 1)]
        rec["eval_speedup"] = round(rec["eval_torch_us"] / rec["eval_ours_us"], 2)
        emit(rec, a.out)


if __name__ == "__main__":
    main()
