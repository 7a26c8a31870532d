#!/usr/bin/env python3
"""bench_eval.py -- GRAND+'s evaluation path, one JSON line per case, on synthetic data.

Not the driver's bench (that is bench.py = GFPush rows/s).  Cases:
  valid_reddit, valid_cora   `valid` over the validation split in mini-batches of the TRAINING batch size, as main() calls
                             it (model.py:345): 23 699 nodes / 50 = 474 batches at reddit, 500 / 50 at cora;
  predict_amazon2m           `predict` over all 2 449 029 nodes, logits 10 000 rows at a time, 80 % of the nodes tested.
ours  = grand_plus_amd.valid / predict: resident rows, one position lookup, the fused head, nothing read back but the
        two scalars (their .item() is inside the timed call, as the reference's is);
torch = the reference's formulation on device tensors: per batch random_prop with index_add_ (the batch's COO tensors are
        built before the clock starts, which the reference pays for on the host every time), the torch MLP,
        log_softmax; then cat, nll_loss, accuracy and two .item(); for predict the same propagate_features call, the torch
        MLP per 10 000 rows, every logit copied to the host, numpy argmax and the comparison there (model.py:212-222).
The two alternate in one process; CUDA events go around each whole call; the median of --reps windows is reported.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as Fn  # noqa: E402

from _bench_steps import emit, synthetic_rows, timed, torch_prop  # noqa: E402
from grand_plus_amd import evaluate  # noqa: E402
from grand_plus_amd.mlp import GrandPlusMLP  # noqa: E402
from grand_plus_amd.rows import RowMatrix  # noqa: E402

# name -> (kind, nodes, F, hidden, classes, layers, use_bn, K, evaluated nodes, batch size)
CASES = {
    "valid_cora": ("valid", 2_708, 1433, 64, 7, 2, False, 32, 500, 50),
    "valid_reddit": ("valid", 232_965, 602, 512, 41, 2, True, 64, 23_699, 50),
    "predict_amazon2m": ("predict", 2_449_029, 100, 1024, 47, 2, True, 0, 1_959_223, 10_000),
}
P_NODE = 0.5


def build_valid(case, dev):
    _, N, F, H, C, nl, bn, K, n_val, B = case
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    model = GrandPlusMLP(F, C, H, nl, bn, 0.0, 0.0, bn).to(dev)
    X = torch.randn((N, F), device=dev)
    labels = torch.randint(0, C, (N,), device=dev)
    seeds = rng.choice(N, n_val, replace=False).astype(np.int64)
    col, val, filled = synthetic_rows(rng, dev, n_val, K, N)
    rm = RowMatrix(seeds, K, None, col, val, filled, N)
    idx_val = rng.permutation(seeds)
    pos = rm.batch_positions(idx_val).long()
    batches = []                                                        # the reference's per-batch tensors, already on the device
    for s in range(0, n_val, B):
        r = pos[s:s + B]
        batches.append((col.view(n_val, K)[r].reshape(-1).long(), val.view(n_val, K)[r].reshape(-1).float(),
                        torch.arange(r.numel(), device=dev).repeat_interleave(K), r.numel()))
    y_val = labels[torch.from_numpy(idx_val).to(dev)]

    def ours():
        loss, acc = evaluate.valid(model, rm, X, idx_val, labels, batch_size=B, dropnode_rate=P_NODE)
        return loss.item(), acc.item()

    def ref():
        model.eval()
        outs = []
        with torch.no_grad():
            for nbr, scores, idx, n_out in batches:
                outs.append(torch.log_softmax(model.reference_forward(torch_prop(X[nbr], scores, idx, P_NODE, False, n_out)), dim=-1))
        outs = torch.cat(outs, dim=0)
        loss = Fn.nll_loss(outs, y_val)
        acc = outs.max(1)[1].eq(y_val).double().sum() / len(y_val)
        return loss.item(), acc.item()

    return ours, ref


def build_predict(case, dev):
    from grand_plus_amd import Graph, synth
    _, N, F, H, C, nl, bn, _K, n_test, B = case
    indptr, indices = synth.shape_csr("amazon2m")
    graph = Graph(indptr, indices, dev.index)
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    model = GrandPlusMLP(F, C, H, nl, bn, 0.0, 0.0, bn).to(dev)
    X = torch.randn((N, F), device=dev)
    labels = torch.randint(0, C, (N,), device=dev)
    idx_test = rng.choice(N, n_test, replace=False).astype(np.int64)
    idx_dev = torch.from_numpy(idx_test).to(dev)

    def ours():
        return evaluate.predict(graph, X, model, idx_dev, labels, "ppr", 2, batch_size_logits=B).item()

    def ref():
        model.eval()
        feat = graph.propagate_features(X, "ppr", 2, 0.2)
        logits = []
        with torch.no_grad():
            for i in range(0, N, B):
                logits.append(model.reference_forward(feat[i:i + B]).to("cpu").numpy())
        preds = np.vstack(logits).argmax(1)
        return float(np.equal(preds[idx_test], labels.cpu().numpy()[idx_test]).sum() / len(idx_test))

    return ours, ref


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for name in a.cases.split(","):
        case = CASES[name]
        fns = dict(zip(("ours", "torch"), (build_valid if case[0] == "valid" else build_predict)(case, dev)))
        results = {k: fn() for k, fn in fns.items()}                   # warms every shape; the two must agree
        rounds = {k: [] for k in fns}
        for _ in range(a.reps):
            for k, fn in fns.items():
                rounds[k].append(timed(fn, 1, 1, warmup=0)[0])
        rec = {"case": name, "nodes": case[1], "evaluated": case[8], "batch": case[9], "reps": a.reps,
               "ours_result": results["ours"], "torch_result": results["torch"]}
        for k, v in rounds.items():
            rec[k + "_ms"] = round(float(np.median(v)) / 1e3, 3)
            rec[k + "_ms_range"] = [round(min(v) / 1e3, 3), round(max(v) / 1e3, 3)]
        rec["speedup_vs_torch"] = round(rec["torch_ms"] / rec["ours_ms"], 2)
        emit(rec, a.out)


if __name__ == "__main__":
    main()
