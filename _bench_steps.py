"""What the side benchmarks of the training step share (bench_train_step.py, bench_mlp_step.py, bench_mag_step.py):
the timing loop, the JSON line, the plain-torch random_prop that is their comparison column, and the synthetic
resident rows.  Not the driver's bench (that is bench.py)."""
import json

import numpy as np
import torch
import torch.nn.functional as Fn


def timed(fn, iters, reps, warmup):
    """(median, min, max) microseconds per call over `reps` windows of `iters` calls, CUDA events around each window."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters * 1e3)                  # microseconds
    return float(np.median(out)), float(min(out)), float(max(out))


def emit(rec, path=None):
    """Prints rec as one JSON line and, with a path, appends it there."""
    line = json.dumps(rec)
    print(line, flush=True)
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def torch_prop(feats, scores, idx, p, training, n_out):
    """The reference's random_prop (model.py:80-87) on device COO tensors, index_add_ for torch_scatter's sum.  The timed
    comparison column: this op sequence stays as it is."""
    s = Fn.dropout(scores, p, training=training)
    num = torch.zeros((n_out, feats.shape[1]), device=feats.device).index_add_(0, idx, feats * s[:, None])
    den = torch.zeros((n_out, 1), device=feats.device).index_add_(0, idx, s[:, None])
    return num / (den + 1e-12)


def synthetic_rows(rng, dev, S_rows, K, n_nodes):
    """Resident [S_rows x K] rows, every slot filled: uniform random neighbours, scores descending: (col, val, filled)."""
    col = torch.from_numpy(rng.integers(0, n_nodes, S_rows * K).astype(np.int32)).to(dev)
    val = torch.from_numpy(np.sort(rng.random((S_rows, K)) ** 4, axis=1)[:, ::-1].copy().reshape(-1)).to(dev)
    filled = torch.full((S_rows,), K, dtype=torch.int32, device=dev)
    return col, val, filled


def batch_of(rng, dev, col, val, S_rows, K, B):
    """A batch of B distinct rows and the reference's tensors for it after its host preparation and upload
    (model.py:310-316): (rows, nbr, scores, idx) = row positions, gathered neighbour ids, scores, output row ids."""
    rows = torch.from_numpy(rng.choice(S_rows, B, replace=False).astype(np.int32)).to(dev)
    r = rows.long()
    nbr = col.view(S_rows, K)[r].reshape(-1).long()
    scores = val.view(S_rows, K)[r].reshape(-1).float()
    idx = torch.arange(B, device=dev).repeat_interleave(K)
    return rows, nbr, scores, idx
