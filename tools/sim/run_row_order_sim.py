#!/usr/bin/env python3
"""What handing rows out heaviest-first is worth at the end of a launch, simulated on the CPU (option "row_order").

Per-row edge counts come from the oracle (one seed per call, one thread), the estimate from grand_plus_amd/row_cost.py (what
row_cost_kernel computes).  List scheduling on `workers` workgroups: a free workgroup takes the next row of the queue; a row
costs a + b * edges microseconds, fitted to 20 us at no edges and 145 us at 27 k (profiles/r06_mag_sk_phases.txt).  Reported
per order: the makespan, and the mean idle time of a workgroup between its last row and the end of the launch.

Usage: python tools/sim/run_row_order_sim.py [workload] [n_seeds] [deg_sat]     (deg_sat: where the device's degree field
saturates on that graph -- 127 on the MAG shape's self-addressed copy; 0 = exact degrees)"""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import bench
from grand_plus_amd.recipes import RECIPES
from grand_plus_amd.row_cost import cost_class, order_by_class, row_costs
from oracle import pyoracle

A_US, B_US = 20.0, (145.0 - 20.0) / 27000.0


def simulate(cost_us, workers):
    """Greedy list scheduling in queue order: (makespan, mean idle behind a worker's last row)."""
    import heapq
    free = [0.0] * workers
    heapq.heapify(free)
    for c in cost_us:
        heapq.heappush(free, heapq.heappop(free) + c)
    free = np.array(free)
    return free.max(), (free.max() - free).mean()


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "small"
    S = int(sys.argv[2]) if len(sys.argv) > 2 else 16384
    sat = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    source, rkey, _ = bench.WORKLOADS[name]
    threads = bench.host_threads()
    ip, ix = bench.load_graph(source, threads)
    r = RECIPES[rkey]
    seeds = bench.make_seeds(source, len(ip) - 1, 65536)[:S].astype(np.int32)      # a sample of the benchmark's own seeds

    def edges_of(i):
        return pyoracle.gfpush(ip, ix, seeds[i:i + 1], r.coef(), r.rmax, r.top_k, threads=1)[3]["edges"]
    with ThreadPoolExecutor(threads) as ex:
        edges = np.array(list(ex.map(edges_of, range(len(seeds)))), np.float64)
    est = row_costs(ip, ix, seeds, r.rmax, sat if sat > 0 else 1 << 30)
    cls = cost_class(est)
    cost = A_US + B_US * edges
    print(f"{name}: {len(seeds)} rows, edges per row mean {edges.mean():.0f} / p50 {np.median(edges):.0f} / p99 {np.percentile(edges, 99):.0f} / max {edges.max():.0f} "
          f"(max / mean {edges.max() / edges.mean():.1f}); degree field saturates at {sat if sat > 0 else 'nothing'}")
    print(f"   estimate (levels 1-2) against the row's edges: rank correlation {np.corrcoef(np.argsort(np.argsort(est)), np.argsort(np.argsort(edges)))[0, 1]:.3f}; "
          f"classes used {np.unique(cls).tolist()}")
    orders = {"caller order": np.arange(len(seeds)), "estimate classes, descending": order_by_class(cls),
              "true edges, descending (the bound)": np.argsort(-edges, kind="stable")}
    for workers, rows in ((512, len(seeds)), (512, min(10400, len(seeds)))):
        print(f"   {workers} workgroups, {rows} rows, cost = {A_US:.0f} + {B_US * 1000:.2f} us per 1 000 edges:")
        for label, o in orders.items():
            o = o[o < rows] if label == "caller order" else np.array([i for i in o if i < rows])
            span, idle = simulate(cost[o], workers)
            print(f"      {label:36s} launch {span / 1000:8.3f} ms   mean idle at the end {idle:7.1f} us = {100 * idle / span:5.2f} %")


if __name__ == "__main__":
    main()
