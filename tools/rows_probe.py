#!/usr/bin/env python3
"""rows_probe.py -- the two window kernels of csrc/optim_rows.hip alone: gp_optim_rows_sqnorm and
gp_clip_adam_rows in lazy mode, launched back to back and timed with HIP events, at the key-list shape of
bench_mag_captured_step.py (V = 500 000, H = 64, 49 920 sorted positions of which 25 600 are live) for four layouts of the
touched rows: random over the table, contiguous, every 16th row, and none (the all-sentinel list, the kernels' floor).
Prints one line per layout; profiles/mag_table_step_rows_probe.txt is its output on one MI355X."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from grand_plus_amd import _native, optim_rows as orows  # noqa: E402

V, H, N_SORTED, LIVE, CALLS = 500_000, 64, 49_920, 25_600, 50


def keys(kind, rng):
    live = {"random": lambda: np.sort(rng.choice(V, LIVE, replace=False)), "contiguous": lambda: np.arange(LIVE),
            "strided16": lambda: np.arange(LIVE) * 16, "sentinel": lambda: np.zeros(0, np.int64)}[kind]()
    return torch.from_numpy(np.concatenate([live, np.full(N_SORTED - len(live), V)]).astype(np.int64)).cuda()


def timed(fn):
    """Microseconds per call over CALLS back-to-back calls, after five to warm up."""
    for _ in range(5):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(CALLS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / CALLS * 1e3


def main():
    L = _native.lib()
    rng = np.random.default_rng(0)
    dW = torch.randn(V, H, device="cuda")
    p, m, v = (torch.rand(V, H, device="cuda") + 0.1 for _ in range(3))
    ws = torch.zeros(1024, dtype=torch.float64, device="cuda")
    norm = torch.zeros((), device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    print(f"V {V} H {H} n_sorted {N_SORTED} live {LIVE}; {CALLS} back-to-back calls, HIP events, us per call")
    for kind in ("random", "contiguous", "strided16", "sentinel"):
        k = keys(kind, rng)
        t_norm = timed(lambda: L.gp_optim_rows_sqnorm(0, k.data_ptr(), N_SORTED, V, H, dW.data_ptr(), 0, ws.data_ptr(), s))
        t_adam = timed(lambda: L.gp_clip_adam_rows(0, p.data_ptr(), m.data_ptr(), v.data_ptr(), dW.data_ptr(), k.data_ptr(), N_SORTED,
                                                   V, H, orows.MODES["lazy"], 0.1, 1e-2, 0.9, 0.999, 1e-8, 0.0, 0.1, 1.0,
                                                   ws.data_ptr(), norm.data_ptr(), s))
        print(f"{kind:<11} gp_optim_rows_sqnorm {t_norm:6.1f}   gp_clip_adam_rows(lazy) {t_adam:6.1f}", flush=True)


if __name__ == "__main__":
    main()
