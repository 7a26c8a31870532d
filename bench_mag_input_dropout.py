#!/usr/bin/env python3
"""bench_mag_input_dropout.py -- a whole MAG training step WITH input dropout, one JSON line.

Not the driver's bench (that is bench.py = GFPush rows/s).  bench_mag_captured_step.py's shape and step (V = 500 000, H = 64,
B = 40, K = 32, S = 2, synthetic bags of mean 20, 2 000 000 nodes) at input_droprate = 0.5, the default of the reference's
run_model.py.  Five variants, alternated window by window in one process:
  eager             the eager composition with host numbers (a host seed, the host weight, ClipAdam's host step count) and the
                    atomic dW: all the project offered at this rate before MagTrainStep(input_dropout=True) -- the yardstick
  replay-atomic     MagTrainStep(capture=True, deterministic=False, input_dropout=True): one graph replay per step; the front end
                    and the atomic backward read the step's seed from device memory
  replay-det        the same with deterministic=True: the per-sample slot gradient and the masked gather of mag_drop
  replay-det-lazy   replay-det with table_step="lazy" (the table in a parameter group of its own with weight_decay = 0)
  replay-det-p0     replay-det on a model at input_droprate = 0 (mag_det's single slot gradient): what the per-sample gather costs
"pays" means more than 5 % under the eager composition's time, the margin pick_choice uses above the box's spread.
Per variant: `<v>_us` wall clock per step (a window of --iters steps between two synchronisations, median [min, max] of
--reps windows) and `<v>_host_us`, the host time per step to enqueue the same window.

The attribute CSR, the table, the rows and the labels are synthetic (uniform random neighbours, scores and attributes).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from _bench_steps import emit  # noqa: E402
from bench_mag_captured_step import ADAM, BASE_SEED, LAM, N_L, N_SELECTIONS, N_U, P_NODE, TEM, WARMUP, C, S, build, window  # noqa: E402
from grand_plus_amd import ClipAdam, MagTrainStep, StepState, mag_trained_parameters  # noqa: E402
from grand_plus_amd._common import step_seed  # noqa: E402
from grand_plus_amd.mlp import MagMLP  # noqa: E402
from grand_plus_amd.objective import grand_plus_loss  # noqa: E402
from grand_plus_amd.step import step_weight  # noqa: E402

P_IN = 0.5
PAYS = 0.05
VARIANTS = ("eager", "replay-atomic", "replay-det", "replay-det-lazy", "replay-det-p0")


def make_model(c, dev, p_in):
    V, n_class, hidden, nlayers, use_bn, _p_in, hidden_droprate, node_norm = c["model_args"]
    torch.manual_seed(0)
    return MagMLP(V, n_class, hidden, nlayers, use_bn, p_in, hidden_droprate, node_norm).to(dev).train()


def variants(c, dev):
    """name -> step(i): one training step on the i-th selection."""
    rm, attrs = c["rm"], c["attrs"]
    out = {}
    m = make_model(c, dev, P_IN)
    opt = ClipAdam(mag_trained_parameters(m), **ADAM)
    pos = rm.batch_positions(np.concatenate([c["idx_train"], c["idx_unlabel"]]), check=True)
    pool_labels = c["labels"][torch.from_numpy(c["idx_train"]).to(dev)]
    tick = [0]

    def eager(i):
        tr, un = c["sels"][i % N_SELECTIONS]
        sel = torch.from_numpy(np.concatenate([tr, un + c["n_train"]])).pin_memory().to(dev, non_blocking=True)
        tick[0] += 1
        seed, w = step_seed(BASE_SEED, tick[0]), float(step_weight(LAM, WARMUP, tick[0]))
        opt.zero_grad(set_to_none=True)
        aug = m.emb_rows(*attrs, rm, batch_rows=pos.index_select(0, sel), samples=S, dropnode_rate=P_NODE, seed=seed)
        loss, _ = grand_plus_loss(m(aug, seed=seed), pool_labels.index_select(0, sel[:N_L]), N_L, w, tem=TEM, kind="l2")
        loss.backward()
        opt.step()

    out["eager"] = eager
    for key, det, table_step, p_in in (("replay-atomic", False, None, P_IN), ("replay-det", True, None, P_IN),
                                       ("replay-det-lazy", True, "lazy", P_IN), ("replay-det-p0", True, None, 0.0)):
        mm = make_model(c, dev, p_in)
        params = mag_trained_parameters(mm)
        if table_step == "lazy":                                    # lazy mode takes no weight decay on the table
            params = [dict(params=params[:1], weight_decay=0.0), dict(params=params[1:])]
        kw = {} if table_step is None else dict(table_step=table_step)
        ts = MagTrainStep(mm, ClipAdam(params, capturable=True, state=StepState(dev), **ADAM), rm, *attrs,
                          c["labels"], c["idx_train"], c["idx_unlabel"], samples=S, dropnode_rate=P_NODE, lam=LAM, warmup=WARMUP,
                          tem=TEM, kind="l2", seed=BASE_SEED, capture=True, deterministic=det, input_dropout=True, **kw)
        out[key] = lambda i, ts=ts: ts.step(*c["sels"][i % N_SELECTIONS])
        out[key].step = ts
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=2_000_000)
    ap.add_argument("--vocab", type=int, default=500_000)
    ap.add_argument("--bag", type=int, default=20, help="attributes per node (each node gets 1 .. 2*bag-1, mean bag)")
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--K", type=int, default=32)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    c = build(a, dev)
    v = variants(c, dev)
    for fn in v.values():                                           # warm-up: code load, optimiser state, the capture
        for i in range(3):
            fn(i)
    torch.cuda.synchronize()
    wall = {k: [] for k in v}
    host = {k: [] for k in v}
    for rep in range(a.reps):
        for k, fn in v.items():                                     # alternated: a drift of the clocks reaches every variant
            w, h = window(fn, a.iters, 3 + rep * a.iters)
            wall[k].append(w)
            host[k].append(h)
    det = v["replay-det"].step
    for k in v:
        if k != "eager":
            v[k].step.check_entries_flag()
    rec = {"case": "mag-train-step-input-dropout", "input_droprate": P_IN, "S": S, "B": N_L + N_U, "K": a.K, "H": a.hidden, "C": C,
           "assumed_vocab": a.vocab, "assumed_bag_mean": a.bag, "assumed_nodes": a.nodes, "longest_bag": det.longest_bag,
           "max_entries": det._max_entries(N_L + N_U), "table_bytes": 4 * a.vocab * a.hidden, "iters": a.iters, "reps": a.reps}
    for k in v:
        key = k.replace("-", "_")
        rec[key + "_us"] = round(float(np.median(wall[k])), 1)
        rec[key + "_us_range"] = [round(min(wall[k]), 1), round(max(wall[k]), 1)]
        rec[key + "_host_us"] = round(float(np.median(host[k])), 1)
        rec[key + "_host_us_range"] = [round(min(host[k]), 1), round(max(host[k]), 1)]
    for k in VARIANTS[1:4]:                                         # against the eager composition at the same rate, in this process
        key = k.replace("-", "_")
        rec[key + "_vs_eager"] = round(rec["eager_us"] / rec[key + "_us"], 3)
        rec[key + "_pays"] = bool(rec[key + "_us"] * (1.0 + PAYS) < rec["eager_us"])
    rec["per_sample_gather_us"] = round(rec["replay_det_us"] - rec["replay_det_p0_us"], 1)
    emit(rec, a.out)


if __name__ == "__main__":
    main()
