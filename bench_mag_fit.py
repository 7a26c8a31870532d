#!/usr/bin/env python3
"""bench_mag_fit.py -- the training loop around a captured MAG step, host-driven against `fit`, and the best-weights
snapshot of the table whole against row by row, one JSON line per case.

Not the driver's bench (that is bench.py = GFPush rows/s).  At bench_mag_captured_step.py's shape (V = 500 000, H = 64,
B = 20 + 20, K = 32, S = 2, synthetic bags of mean 20, 2 000 000 nodes), the lazy table step over the atomic backward with
its bitmap row list ("atomic") and over the deterministic backward ("det"), 500 validation nodes in batches of 100, a
validation every 10 steps.

(a) case "mag-fit-loop-<mode>": three loops alternated window by window in one process:
  host       what a caller could write before `fit` took a MagTrainStep: `step_sampled`; every 10 steps `valid_mag` (the node
             ids uploaded and looked up again), two `.item()`s and the early-stop rule in Python, and on an improvement a
             device clone of the state_dict (the 128 MB table with it; no file is written)
  fit        `fit`'s loop, the table snapshotted whole (gp_fit_snapshot), polled at every validation
  fit_dirty  the same over a step built with dirty_rows=True: the table snapshotted row by row
Per loop `<loop>_wall_us`, wall clock per step of a window (validations included, the GPU drained at its end), and
`<loop>_host_us`, the host time per step to get the window enqueued; each the median over --reps windows with the
window-to-window range beside it -- the noise floor of this same-process comparison.  Labels are random, so improvements are
rare: this part prices the loop, not the snapshot.

(b) case "mag-fit-snapshot-<mode>": `tracker.update` driven with a scripted accuracy that never falls under
stop_mode="acc", so that every update copies; 10 training steps between two updates mark the rows a snapshot has to copy.
`full` copies the table whole, `dirty` the marked rows.  Per path `<path>_update_us`, the device time of one update (the
rule, the snapshot of the layers and the table's) between two events, and `<path>_cycle_us`, wall clock of 10 steps and one
update in a window drained at its end; `dirty_rows_marked` is the number of rows a snapshot found marked.

The attribute CSR, the table, the rows and the labels are synthetic (uniform random neighbours, scores and attributes).
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from _bench_steps import emit, synthetic_rows  # noqa: E402
from grand_plus_amd import ClipAdam, MagTrainStep, Sampler, StepState, mag_trained_parameters, valid_mag  # noqa: E402
from grand_plus_amd.fit import BestTracker, FitLoop, early_stop_rule, new_track  # noqa: E402
from grand_plus_amd.mlp import MagMLP  # noqa: E402
from grand_plus_amd.rows import RowMatrix  # noqa: E402

S, P_NODE, TEM, C, N_L, N_U = 2, 0.5, 0.5, 8, 20, 20
LAM, WARMUP, BASE_SEED, EVAL_BATCH, PATIENCE = 1.0, 100, 0x5EED, 10, 10 ** 9
N_VAL, VALID_BATCH = 500, 100
ADAM = dict(lr=1e-2, weight_decay=5e-4, clip_norm=0.1)
MODES = {"atomic": dict(deterministic=False, row_list="bitmap"), "det": dict(deterministic=True)}


def build(a, dev):
    rng = np.random.default_rng(0)
    N, V, K = a.nodes, a.vocab, a.K
    lens = rng.integers(1, 2 * a.bag, N)
    indptr = np.zeros(N + 1, np.int64)
    np.cumsum(lens, out=indptr[1:])
    indices = rng.integers(0, V, int(indptr[-1])).astype(np.int32)
    data = (rng.random(int(indptr[-1]), dtype=np.float32) + 0.05).astype(np.float32)
    attrs = tuple(torch.from_numpy(x).to(dev) for x in (indptr, indices, data))
    S_rows = 20_000
    seeds = rng.choice(N, S_rows, replace=False).astype(np.int64)
    col, val, filled = synthetic_rows(rng, dev, S_rows, K, N)
    row = torch.from_numpy(np.repeat(seeds, K).astype(np.int32)).to(dev)
    n_train = S_rows // 10
    return dict(rm=RowMatrix(seeds, K, row, col, val, filled, N), attrs=attrs, labels=torch.from_numpy(rng.integers(0, C, N)).to(dev),
                idx_train=seeds[:n_train], idx_val=seeds[n_train:n_train + N_VAL], idx_unlabel=seeds[n_train + N_VAL:],
                model_args=(V, C, a.hidden, 2, True, 0.0, 0.5, True))


def train_step(c, dev, mode, dirty_rows=False):
    torch.manual_seed(0)
    m = MagMLP(*c["model_args"]).to(dev).train()
    params = mag_trained_parameters(m)
    params = [dict(params=params[:1], weight_decay=0.0), dict(params=params[1:])]   # lazy mode takes no weight decay on the table
    opt = ClipAdam(params, capturable=True, state=StepState(dev), **ADAM)
    return MagTrainStep(m, opt, c["rm"], *c["attrs"], c["labels"], c["idx_train"], c["idx_unlabel"], samples=S, dropnode_rate=P_NODE,
                        lam=LAM, warmup=WARMUP, tem=TEM, kind="l2", seed=BASE_SEED, capture=True, table_step="lazy",
                        dirty_rows=dirty_rows, **MODES[mode])


def sampler(ts):
    return Sampler(ts.n_train, ts.n_unlabel, N_L, N_U, BASE_SEED)


class HostLoop:
    """The loop of before: the step sampled on the device, every validation planned anew and read back, the rule and the
    checkpoint on the host."""

    def __init__(self, c, dev, mode):
        self.c, self.ts = c, train_step(c, dev, mode)
        self.sampler = sampler(self.ts)
        self.t, self.track, self.saved = 0, new_track(), None

    def advance(self):
        c = self.c
        self.t += 1
        self.ts.step_sampled(self.sampler, self.t)
        if (self.t - 1) % EVAL_BATCH == 0:
            loss, acc = valid_mag(self.ts.model, c["rm"], *c["attrs"], c["idx_val"], c["labels"], batch_size=VALID_BATCH,
                                  dropnode_rate=P_NODE)
            early_stop_rule(self.track, loss.item(), acc.item(), self.t, "both", PATIENCE)
            if self.track["copy_now"]:
                self.saved = {k: v.clone() for k, v in self.ts.model.state_dict().items()}


class FitRun:
    """`fit`'s loop body over a FitLoop that outlives a window."""

    def __init__(self, c, dev, mode, dirty_rows):
        ts = train_step(c, dev, mode, dirty_rows)
        self.loop = FitLoop(ts, sampler(ts), c["idx_val"], eval_batch=EVAL_BATCH, stop_mode="both", patience=PATIENCE,
                            valid_batch=VALID_BATCH)

    def advance(self):
        loop = self.loop
        if loop.advance() and loop.poll().stopped:
            raise RuntimeError("the run stopped early: patience is meant to be out of reach")


class SnapshotRun:
    """Ten steps, then one `tracker.update` that copies: the accuracy fed to the rule never falls."""

    def __init__(self, c, dev, mode, dirty_rows, n_updates):
        self.ts = train_step(c, dev, mode, dirty_rows)
        self.sampler = sampler(self.ts)
        self.tracker = BestTracker(self.ts.model, dev, "acc", PATIENCE, row_grad=self.ts.row_grad if dirty_rows else None)
        vals = torch.zeros((n_updates, 2), dtype=torch.float32)
        vals[:, 0] = 1.0
        vals[:, 1] = torch.arange(n_updates) / n_updates               # the scripted accuracy
        self.vals = vals.to(dev)
        self.t = self.u = 0
        self.events = []

    def advance(self, timed=False):
        for _ in range(EVAL_BATCH):
            self.t += 1
            self.ts.step_sampled(self.sampler, self.t)
        v = self.vals[self.u]
        self.u += 1
        if timed:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        self.tracker.update(v[0], v[1], self.ts.state)
        if timed:
            e1.record()
            self.events.append((e0, e1))

    def marked(self):
        """The rows the next snapshot would copy (a host read: outside every window)."""
        d = self.ts.row_grad.dirty
        return int(sum(bin(int(w) & 0xFFFFFFFF).count("1") for w in d.cpu().numpy())) if d is not None else None


def window(advance, iters):
    """(wall, host) microseconds per call over one window of `iters` calls."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        advance()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6, host / iters * 1e6


def _stats(rec, key, xs):
    rec[key] = round(float(np.median(xs)), 1)
    rec[key + "_range"] = [round(min(xs), 1), round(max(xs), 1)]


def loop_case(c, dev, mode, a, base):
    runs = {"host": HostLoop(c, dev, mode), "fit": FitRun(c, dev, mode, False), "fit_dirty": FitRun(c, dev, mode, True)}
    n_batches = -(-len(c["idx_train"]) // N_L)
    for run in runs.values():                                       # warm-up: code load, the capture, a few validations
        for _ in range(3 * EVAL_BATCH + 2):
            run.advance()
    torch.cuda.synchronize()
    wall = {k: [] for k in runs}
    host = {k: [] for k in runs}
    for _rep in range(a.reps):
        for k, run in runs.items():                                 # alternated: a drift of the clocks reaches all three
            w, h = window(run.advance, a.iters)
            wall[k].append(w)
            host[k].append(h)
    rec = dict(base, case=f"mag-fit-loop-{mode}", n_batches=n_batches, iters=a.iters, reps=a.reps,
               fit_best_tick=runs["fit"].loop.poll().best_tick, fit_dirty_best_tick=runs["fit_dirty"].loop.poll().best_tick,
               host_best_tick=int(runs["host"].track["best_tick"]))
    for k in runs:
        _stats(rec, k + "_wall_us", wall[k])
        _stats(rec, k + "_host_us", host[k])
    for k in ("fit", "fit_dirty"):
        rec[k + "_speedup_vs_host"] = round(rec["host_wall_us"] / rec[k + "_wall_us"], 3)
    for run in runs.values():
        (run.ts if isinstance(run, HostLoop) else run.loop.step).check_entries_flag()
    emit(rec, a.out)


def snapshot_case(c, dev, mode, a, base):
    n = 3 + a.reps * a.updates + 1
    runs = {"full": SnapshotRun(c, dev, mode, False, n), "dirty": SnapshotRun(c, dev, mode, True, n)}
    for run in runs.values():
        for _ in range(3):
            run.advance()
    torch.cuda.synchronize()
    cycle = {k: [] for k in runs}
    marked = []
    for _rep in range(a.reps):
        for k, run in runs.items():
            w, _h = window(lambda run=run: run.advance(timed=True), a.updates)
            cycle[k].append(w)
    for _ in range(EVAL_BATCH):                                     # what one more snapshot would find marked
        runs["dirty"].t += 1
        runs["dirty"].ts.step_sampled(runs["dirty"].sampler, runs["dirty"].t)
    marked.append(runs["dirty"].marked())
    torch.cuda.synchronize()
    rec = dict(base, case=f"mag-fit-snapshot-{mode}", steps_between_updates=EVAL_BATCH, updates=a.updates, reps=a.reps,
               dirty_rows_marked=marked[0], table_rows=c["model_args"][0])
    for k, run in runs.items():
        image = run.tracker.read()
        if image.best_tick != run.t - (EVAL_BATCH if k == "dirty" else 0) or image.n_evals != run.u:
            raise RuntimeError(f"{k}: an update did not take a new best (best_tick {image.best_tick}, step {run.t})")
        _stats(rec, k + "_update_us", [e0.elapsed_time(e1) * 1e3 for e0, e1 in run.events])
        _stats(rec, k + "_cycle_us", cycle[k])
    rec["dirty_update_speedup_vs_full"] = round(rec["full_update_us"] / rec["dirty_update_us"], 2)
    w, snap = runs["dirty"].ts.model.embeds.weight.detach(), runs["dirty"].tracker._table[1]
    clean = torch.ones(w.shape[0], dtype=torch.bool, device=dev)
    # the invariant, at the size timed: every row the last ten steps did not mark has the same bits in the table and its snapshot
    d = runs["dirty"].ts.row_grad.dirty
    bits = (d.view(torch.int32)[:, None] >> torch.arange(32, device=dev, dtype=torch.int32)[None, :]) & 1
    clean &= bits.reshape(-1)[:w.shape[0]] == 0
    if not torch.equal(w[clean].view(torch.int32), snap[clean].view(torch.int32)):
        raise RuntimeError("a row whose dirty bit is 0 differs between the table and its snapshot")
    emit(rec, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=2_000_000)
    ap.add_argument("--vocab", type=int, default=500_000)
    ap.add_argument("--bag", type=int, default=20, help="attributes per node (each node gets 1 .. 2*bag-1, mean bag)")
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--K", type=int, default=32)
    ap.add_argument("--modes", default="atomic,det")
    ap.add_argument("--iters", type=int, default=800, help="steps per window of part (a)")
    ap.add_argument("--updates", type=int, default=40, help="updates per window of part (b), ten steps before each")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parts", default="a,b")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    c = build(a, dev)
    base = {"S": S, "B": N_L + N_U, "K": a.K, "H": a.hidden, "C": C, "assumed_vocab": a.vocab, "assumed_bag_mean": a.bag,
            "assumed_nodes": a.nodes, "n_val": N_VAL, "valid_batch": VALID_BATCH, "eval_batch": EVAL_BATCH,
            "table_bytes": 4 * a.vocab * a.hidden}
    for mode in a.modes.split(","):
        if "a" in a.parts.split(","):
            loop_case(c, dev, mode, a, base)
        if "b" in a.parts.split(","):
            snapshot_case(c, dev, mode, a, base)


if __name__ == "__main__":
    main()
