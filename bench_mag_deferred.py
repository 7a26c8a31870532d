#!/usr/bin/env python3
"""bench_mag_deferred.py -- MAG's captured step with the table stepped "exact", "lazy" and "deferred" (DESIGN.md §7za), one JSON
line per id distribution.

Not the driver's bench (that is bench.py = GFPush rows/s).  At bench_mag_captured_step.py's shape (V = 500 000, H = 64, B = 40,
K = 32, S = 2, synthetic bags of mean 20, 2 000 000 nodes) and with its build, the three table steps on both backwards
(det: the sort-then-gather dW; atomic: row_list="bitmap"), alternated window by window in one process, in two regimes:
  bare      the replayed step alone: `<mode>_<backward>_us`;
  flush10   the step with flush_table() after every 10th step, which is what `fit` does at eval_batch = 10:
            `deferred_<backward>_flush10_us`.  For "exact" and "lazy" flush_table() launches nothing, so their bare figure stands.
The table sits in a parameter group of its own with weight_decay = 0, which "lazy" requires, in every variant alike.
Per deferred variant also, each alone between CUDA events after 10 steps of lag, median [min, max] of --reps:
`_flush_us` (one flush_table()), `_list_us` (the pre-forward row list: mark + compact) and `_catch_up_us` (the catch-up launch
of the next batch's rows), and `_lagging_rows`, the rows the last flush found behind.
--ids uniform | zipf | both: the attribute ids of the bags uniform over V or bench_det_chunk.py's Zipf ids (probability
proportional to 1 / rank): they change how many rows lag and by how much.
Wall clock per step: a window of --iters steps between two synchronisations, median [min, max] of --reps windows.
--profile-variant <variant> runs that one variant for --iters steps after its warm-up, for a kernel trace run of its own.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench_mag_captured_step as cs  # noqa: E402
from _bench_steps import emit  # noqa: E402
from bench_det_chunk import zipf_ids  # noqa: E402
from grand_plus_amd import ClipAdam, MagTrainStep, StepState, mag_trained_parameters  # noqa: E402

MODES = ("exact", "lazy", "deferred")
BACKWARDS = ("det", "atomic")
FLUSH_EVERY = 10
VARIANTS = tuple(f"{m}-{b}" for b in BACKWARDS for m in MODES)


def make_step(c, dev, attrs, mode, backward, capacity):
    mm = cs.make_model(c, dev)
    params = mag_trained_parameters(mm)
    params = [dict(params=params[:1], weight_decay=0.0), dict(params=params[1:])]
    kw = dict(table_step=mode)
    if backward == "atomic":
        kw["row_list"] = "bitmap"
    if mode == "deferred":
        kw["defer_capacity"] = capacity
    return MagTrainStep(mm, ClipAdam(params, capturable=True, state=StepState(dev), **cs.ADAM), c["rm"], *attrs, c["labels"],
                        c["idx_train"], c["idx_unlabel"], samples=cs.S, dropnode_rate=cs.P_NODE, lam=cs.LAM, warmup=cs.WARMUP,
                        tem=cs.TEM, kind="l2", seed=cs.BASE_SEED, capture=True, deterministic=backward == "det", **kw)


def events(fn, before, reps):
    """Microseconds of fn() alone between two CUDA events, `reps` times, before() run ahead of each: (median, min, max)."""
    out = []
    for _ in range(reps):
        before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return round(float(np.median(out)), 1), [round(min(out), 1), round(max(out), 1)]


def run(a, dev, c, ids):
    ip, ix, dt = c["attrs"]
    if ids == "zipf":
        ix = torch.from_numpy(zipf_ids(a.vocab)(np.random.default_rng(1), ix.numel()).astype(np.int32)).to(dev)
    attrs = (ip, ix, dt)
    sels = c["sels"]
    steps, fns = {}, {}
    for name in VARIANTS if a.profile_variant is None else (a.profile_variant,):
        mode, backward = name.split("-")
        steps[name] = ts = make_step(c, dev, attrs, mode, backward, a.capacity)
        fns[name] = lambda i, ts=ts: ts.step(*sels[i % cs.N_SELECTIONS])
        if mode == "deferred" and a.profile_variant is None:
            steps[name + "-flush10"] = ts10 = make_step(c, dev, attrs, mode, backward, a.capacity)

            def with_flush(i, ts=ts10):
                ts.step(*sels[i % cs.N_SELECTIONS])
                if i % FLUSH_EVERY == 0:
                    ts.flush_table()
            fns[name + "-flush10"] = with_flush
    for fn in fns.values():                                         # warm-up: code load, optimiser state, the capture
        for i in range(3):
            fn(i)
    torch.cuda.synchronize()
    if a.profile_variant:
        for i in range(a.iters):
            fns[a.profile_variant](3 + i)
        torch.cuda.synchronize()
        return
    wall = {k: [] for k in fns}
    for rep in range(a.reps):
        for k, fn in fns.items():                                   # alternated: a drift of the clocks reaches every variant
            wall[k].append(cs.window(fn, a.iters, 3 + rep * a.iters)[0])
    rec = {"case": "mag-deferred", "ids": ids, "S": cs.S, "B": cs.N_L + cs.N_U, "K": a.K, "H": a.hidden, "assumed_vocab": a.vocab,
           "assumed_bag_mean": a.bag, "assumed_nodes": a.nodes, "defer_capacity": a.capacity, "flush_every": FLUSH_EVERY,
           "table_bytes": 4 * a.vocab * a.hidden, "iters": a.iters, "reps": a.reps}
    for k in fns:
        key = k.replace("-", "_")
        rec[key + "_us"] = round(float(np.median(wall[k])), 1)
        rec[key + "_us_range"] = [round(min(wall[k]), 1), round(max(wall[k]), 1)]
    at = [3 + a.reps * a.iters]
    for backward in BACKWARDS:                                      # the flush, the list and the catch-up, each alone
        ts, key = steps[f"deferred-{backward}"], f"deferred_{backward}"

        def lag(ts=ts):
            for _ in range(FLUSH_EVERY):
                ts.step(*sels[at[0] % cs.N_SELECTIONS])
                at[0] += 1

        ts.flush_table()
        lagging = []

        def lag_and_count(ts=ts):
            lag()
            lagging.append(int((ts.deferred.last != int(ts.state.read().tick)).sum()))

        rec[key + "_flush_us"], rec[key + "_flush_us_range"] = events(ts.flush_table, lag_and_count, a.reps)
        rec[key + "_lagging_rows"] = lagging[-1]
        rows, B = c["rm"], cs.N_L + cs.N_U
        batch = [None]

        def next_batch(ts=ts):
            lag()
            tr, un = sels[at[0] % cs.N_SELECTIONS]
            sel = torch.from_numpy(np.concatenate([tr, un + c["n_train"]])).to(dev)
            batch[0] = ts._pos.index_select(0, sel)

        def listing(ts=ts):
            V = ts.model.embeds.weight.shape[0]
            return ts.deferred.list_batch(attrs[0], attrs[1], rows.col, rows.filled, rows.col.numel() // rows.K, rows.K, batch[0],
                                          min(V, ts._max_entries(B)), ts._entries_flag)

        rec[key + "_list_us"], rec[key + "_list_us_range"] = events(listing, next_batch, a.reps)
        keys = [None]

        def listed(ts=ts):
            next_batch()
            keys[0] = listing()

        rec[key + "_catch_up_us"], rec[key + "_catch_up_us_range"] = events(lambda ts=ts: ts.deferred.catch_up(keys[0]), listed, a.reps)
        rec[key + "_listed_rows"] = int((keys[0] < a.vocab).sum())
    for ts in steps.values():
        ts.check_entries_flag()
    emit(rec, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=2_000_000)
    ap.add_argument("--vocab", type=int, default=500_000)
    ap.add_argument("--bag", type=int, default=20, help="attributes per node (each node gets 1 .. 2*bag-1, mean bag)")
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--K", type=int, default=32)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--capacity", type=int, default=1024, help="defer_capacity of the deferred variants")
    ap.add_argument("--ids", default="both", choices=("uniform", "zipf", "both"))
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--profile-variant", default=None, choices=VARIANTS, help="warm it up, then run it --iters times")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    c = cs.build(a, dev)
    for ids in ("uniform", "zipf") if a.ids == "both" else (a.ids,):
        run(a, dev, c, ids)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
