"""The shell applies the plan: after the calls of a recorded case (tests/golden/gfpush_plans.json, recorded from the parent of the
commit that moved the decisions into csrc/gfpush_plan.hpp) gp_stats reports the recorded kernel, workgroups, block size, LDS
and workspace bytes.  4 096 rows at the most: below the 32 768 rows that trigger a calibration, so nothing is timed."""
import pytest

import plan_cases

pytestmark = pytest.mark.gpu

DOC = plan_cases.load()


@pytest.mark.parametrize("case", DOC["cases"], ids=[c["id"] for c in DOC["cases"]])
def test_the_library_runs_the_recorded_plan(case):
    import torch
    assert torch.cuda.get_device_properties(0).multi_processor_count == DOC["num_cus"]      # the recording's device
    got = plan_cases.run_case(case)
    assert len(got) == len(case["expect"])
    for i, (g, want) in enumerate(zip(got, case["expect"])):
        assert {k: g[k] for k in plan_cases.PLAN_FIELDS} == {k: want[k] for k in plan_cases.PLAN_FIELDS}, (case["id"], i, g, want)
        assert g["failed_rows"] == 0
