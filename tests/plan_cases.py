"""The cases of tests/golden/gfpush_plans.json: how a case of that file is run on the GPU (tests/test_gpu_plan.py) and
how it is laid out for the stand-alone planner check (tests/test_host_gfpush_plan.py)."""
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gfpush_plans.json")

# the six gp_stats fields that describe the plan of a call
PLAN_FIELDS = ("kernel", "workgroups", "block_threads", "lds_bytes", "lds_slots", "workspace_bytes")


def load():
    with open(GOLDEN) as f:
        return json.load(f)


def coef_of(call):
    from grand_plus_amd.recipes import make_coef
    return make_coef(call["mode"], call["order"], call["alpha"])


def run_case(case):
    """The case's calls on one fresh handle: per call the PLAN_FIELDS of gp_stats and failed_rows."""
    import numpy as np
    import torch
    from grand_plus_amd import Graph, synth
    indptr, indices = synth.shape_csr(case["graph"])
    g = Graph(indptr, indices, 0)
    try:
        for k, v in case["options"].items():
            g.set_option(k, v)
        out = []
        for call in case["calls"]:
            n = len(indptr) - 1                                     # (more rows than nodes: the seeds repeat)
            seeds = torch.from_numpy(np.resize(synth.seeds(n, min(call["rows"], n)), call["rows"])).to(torch.device("cuda", g.device))
            g.gfpush_device(seeds, coef_of(call), call["rmax"], call["K"])
            st = g.stats()
            out.append({k: int(st[k]) for k in PLAN_FIELDS + ("failed_rows",)})
        return out
    finally:
        g.close()
