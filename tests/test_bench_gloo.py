"""bench.py's multi-rank orchestration on CPU: `--gpus 2` rank code end to end under gloo -- sharding of every
step's batch, the fixed warm-up, the fences, the gather, the max-over-ranks reductions, ONE JSON line on rank 0 -- with the
compute swapped for the CPU oracle: this test passes its own `platform` (Graph class, events, device) to bench.run_rank.  The product
Graph class is not involved: this pins the launcher contract before an 8-GPU driver run meets it."""
import json
import os
import socket
import sys

import numpy as np
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


class _OracleGraph:
    """Stand-in with the slice of grand_plus_amd.api.Graph that bench.run_rank uses; rows come from the CPU oracle."""

    def __init__(self, indptr, indices, seed, device=0):
        self.indptr, self.indices = indptr, indices
        self._st = None
        self.reset_stats()

    def set_option(self, key, value):
        pass

    def reset_stats(self):
        self._st = {k: 0 for k in ("rows", "pushes", "edges", "filled", "support", "frontier", "lds_levels", "global_levels", "failed_rows",
                                   "degree_lookups", "retried_rows", "max_level_edges", "max_log_records", "workspace_bytes",
                                   "sketch_candidate_edges", "sketch_second_sweeps", "diag_ticks_total")}
        self._st.update(kernel_ms=0.0, workgroups=1, block_threads=64, lds_bytes=0, lds_slots=0, kernel=1, diag_sub=[0] * 16)

    def gfpush_device(self, seeds, coef, rmax, K, row, col, val, filled):
        from oracle import pyoracle
        s = seeds.numpy()
        r, c, v, st = pyoracle.gfpush(self.indptr, self.indices, s, coef, rmax, K)
        nf = (v.reshape(len(s), K) > 0).sum(1)
        row[:len(s) * K] = torch.from_numpy(r); col[:len(s) * K] = torch.from_numpy(c)
        val[:len(s) * K] = torch.from_numpy(v); filled[:len(s)] = torch.from_numpy(nf.astype(np.int32))
        self._st["rows"] += len(s); self._st["pushes"] += int(st["pushes"]); self._st["edges"] += int(st["edges"]); self._st["filled"] += int(st["filled"])

    def stats(self):
        return dict(self._st)


class _HostEvent:
    """torch.cuda.Event stand-in (perf_counter stamps)."""
    def __init__(self):
        self.t = 0.0

    def record(self):
        import time
        self.t = time.perf_counter()

    def elapsed_time(self, other):
        return (other.t - self.t) * 1e3


class _CpuPlatform:
    """The stand-in for bench.CudaPlatform: CPU tensors, host clocks, the oracle-backed Graph above."""
    name = "cpu test stand-in"
    graph_class = staticmethod(lambda: _OracleGraph)
    event = staticmethod(lambda: _HostEvent())
    device = staticmethod(lambda local_rank: torch.device("cpu"))
    sync = staticmethod(lambda dev: None)


def _rank(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK=str(rank),
                      GRANDPLUS_BENCH_BACKEND="gloo")
    import bench
    sys.argv = ["bench.py", "--gpus", str(world), "--steps", "2", "--warmup", "1", "--prewarm", "2", "--workload", "pubmed",
                "--seeds-per-gpu", "96", "--no-cpu-baseline", "--no-host-api", "--no-next-rows"]
    out = open(os.path.join(out_dir, f"rank{rank}.out"), "w")
    sys.stdout = out
    rc = bench.run_rank(bench.parse_args(), platform=_CpuPlatform)
    out.flush()
    assert rc == 0


def test_bench_two_ranks_under_gloo_print_one_json_line(tmp_path):
    world = 2
    mp.spawn(_rank, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    lines0 = [ln for ln in open(tmp_path / "rank0.out").read().splitlines() if ln.startswith("{")]
    lines1 = [ln for ln in open(tmp_path / "rank1.out").read().splitlines() if ln.startswith("{")]
    assert len(lines0) == 1 and not lines1                      # rank 0 prints ONE line, the others none
    line = json.loads(lines0[0])
    assert line["n_gpus"] == 2 and line["steps"] == 2 and line["warmup"] == 1 and line["warmup_effective"] == 3
    assert line["scaling"] == "weak" and line["unit"] == "rows/s" and line["value"] > 0 and line["anomaly"] is False
    assert line["config"]["rows_per_step"] == 192 and line["config"]["seeds_per_gpu"] == 96
    assert len(line["kernel_ms_per_rank"]) == 2 and line["rccl_ranks"] == 0        # gloo stand-in, not RCCL
    assert abs(line["value"] - 192 * 2 / (line["ms_per_step"] * 2 * 1e-3)) < 1e-3 * line["value"]
    assert "roofline" in line and line["roofline"]["bound"] == "hbm" and line["vs_baseline"] is None


def test_bench_has_no_cpu_path_of_its_own(monkeypatch):
    """bench.py selects nothing but the product: with the default platform and no GPU the rank stops at GP_ERR_NO_DEVICE."""
    import pytest
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the default platform would run the benchmark")
    sys.path.insert(0, ROOT)
    import bench
    assert not hasattr(bench, "_GRAPH_FACTORY") and "GRANDPLUS_BENCH_DEVICE" not in open(bench.__file__).read()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--workload", "pubmed", "--seeds-per-gpu", "8", "--steps", "1", "--warmup", "0"])
    assert bench.run_rank(bench.parse_args()) == 3


def _plain_run(tmp_path, monkeypatch, capsys, extra=()):
    """One rank, no launcher, the CPU stand-in platform: returns the JSON line and the dump directory."""
    sys.path.insert(0, ROOT)
    import bench
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    out = tmp_path / "dump"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--prewarm", "0", "--workload", "pubmed",
                                      "--seeds-per-gpu", "64", "--dump-outputs", str(out)] + list(extra))
    assert bench.run_rank(bench.parse_args(), platform=_CpuPlatform) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return bench, json.loads(lines[0]), out


def test_bench_plain_run_is_lean_and_dumps_the_last_steps_rows(tmp_path, monkeypatch, capsys):
    """A plain run prints the headline line without the --full blocks, and --dump-outputs writes exactly the rows the last
    timed step computed, in the canonical form of bench.canonical_rows, as float64 .npy files."""
    bench, line, out = _plain_run(tmp_path, monkeypatch, capsys)
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["full"] is False
    for k in ("metric", "value", "unit", "higher_is_better", "dtype"):
        assert k in line
    assert not {"host_api", "cold_call", "next_rows", "cpu_baseline"} & set(line)
    from grand_plus_amd import RECIPES
    from oracle import pyoracle
    source, rkey, _ = bench.WORKLOADS["pubmed"]
    recipe = RECIPES[rkey]
    K = recipe.top_k
    indptr, indices = bench.load_graph(source, 1)
    seeds = bench.make_seeds(source, len(indptr) - 1, 64 * 4)[3 * 64:]          # step 4 of 4 (1 warm-up + 3 timed)
    r, c, v, _ = pyoracle.gfpush(indptr, indices, seeds, recipe.coef(), recipe.rmax, K)
    got = {n: np.load(out / f"{n}.npy") for n in ("row", "col", "val", "filled")}
    assert sorted(os.listdir(out)) == ["col.npy", "filled.npy", "row.npy", "val.npy"]
    assert all(a.dtype == np.float64 for a in got.values())
    nf = (v.reshape(64, K) > 0).sum(1)
    keep = np.arange(K)[None, :] < nf[:, None]
    np.testing.assert_array_equal(got["filled"], nf)
    for i in range(64):
        n = nf[i]
        exp_c, exp_v = c[i * K:i * K + n], v[i * K:i * K + n]
        np.testing.assert_array_equal(got["val"][i, :n], np.sort(exp_v)[::-1])          # (this row set has no near-ties)
        np.testing.assert_array_equal(got["row"][i, :n], r[i * K:i * K + n])
        kth = exp_v.min()
        tied = np.abs(exp_v - kth) <= bench.TIE_RTOL * kth
        if n == K:                                                          # a full row: the K-th value's tie group has no column
            assert (got["col"][i, :n] == -1).sum() == tied.sum()
            np.testing.assert_array_equal(np.sort(got["col"][i, :n][got["col"][i, :n] >= 0]), np.sort(exp_c[~tied]))
        else:
            np.testing.assert_array_equal(np.sort(got["col"][i, :n]), np.sort(exp_c))
        for name in ("row", "col", "val"):
            assert not got[name][i, n:].any()
    assert (np.diff(np.where(keep, got["val"], 0), axis=1) <= 0).all()


def test_bench_dump_form_does_not_depend_on_slot_order_rounding_or_tie_choice():
    """Two launches that return the same rows up to slot order, last-bit noise in the sums and which member of a K-th-value
    tie group is kept dump the same arrays up to that noise; a real difference in a determined column still shows."""
    sys.path.insert(0, ROOT)
    import bench
    K = 4
    filled = np.array([4, 4, 2])
    row = np.repeat([0, 1, 2], K)
    a_col, a_val = np.array([5, 3, 7, 1, 10, 11, 12, 13, 8, 6, 99, 99]), np.array([.5, .3, .1, .2, .4, .3, .2, .1, .2, .3, 9, 9])
    b_col = np.array([9, 1, 3, 5, 13, 12, 11, 10, 6, 8, 42, 42])           # row 0 keeps node 9 instead of the tied node 7
    b_val = np.array([.1 * (1 + 1e-15), .2, .3 * (1 - 2e-15), .5, .1, .2, .3, .4, .3, .2, 7, 7])
    got_a = bench.canonical_rows(row, a_col, a_val, filled, K)
    got_b = bench.canonical_rows(row, b_col, b_val, filled, K)
    for x, y in zip(got_a, got_b):
        assert x.dtype == np.float64 and x.shape == (3, K)
        np.testing.assert_allclose(x, y, rtol=1e-14, atol=0)
    np.testing.assert_array_equal(got_a[1], [[5, 3, 1, -1], [10, 11, 12, -1], [6, 8, 0, 0]])
    np.testing.assert_array_equal(got_a[2], [[.5, .3, .2, .1], [.4, .3, .2, .1], [.3, .2, 0, 0]])
    b_col[1] = 2                                                            # a determined column that differs
    assert not np.array_equal(bench.canonical_rows(row, b_col, b_val, filled, K)[1], got_a[1])


def test_bench_dump_keeps_a_fixed_sample_under_the_byte_budget(tmp_path, monkeypatch, capsys):
    """Above the budget the dump is a seeded sample of rows, the same from run to run, with the rows' positions beside it."""
    import bench
    K = 16                                                                  # the pubmed recipe's top-k
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 8 * (3 * K + 1) * 20)
    _, _, out = _plain_run(tmp_path, monkeypatch, capsys)
    full = tmp_path / "unsampled"
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 64 * 2**20)
    _plain_run(tmp_path, monkeypatch, capsys, ["--dump-outputs", str(full)])
    pick = np.load(out / "sample_rows.npy").astype(np.int64)
    assert len(pick) == 20 and (np.diff(pick) > 0).all() and pick[-1] < 64
    for n in ("row", "col", "val", "filled"):
        np.testing.assert_array_equal(np.load(out / f"{n}.npy"), np.load(full / f"{n}.npy")[pick])
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) < 64 * 2**20
