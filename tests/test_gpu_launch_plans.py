"""ops.conv() launches the tiny workloads exactly as recorded: the launches of tests/golden/igemm_launch_plans.json.gz (written by
tools/record_launch_plans.py on the commit before the planner moved into igemm_plan.py) are recorded again in this process and compared
record for record, in launch order -- the call as asked, the route, the key, the epilogue form, every scalar of the argument struct and
which of its pointers are set."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
FIXTURE = os.path.join(ROOT, "tests", "golden", "igemm_launch_plans.json.gz")


@pytest.mark.gpu
def test_tiny_workloads_launch_as_recorded():
    import record_launch_plans as R
    from audioldm_with_lora_amd import ops
    want = R.load_fixture(FIXTURE)["tuned" if ops.TUNED else "no_tuned"]
    got = json.loads(json.dumps(R.record(("tiny",))))
    assert sorted(got["workloads"]) == sorted(n for n in want["workloads"] if n.startswith("tiny_")) and len(got["workloads"]) == 7
    for name in got["workloads"]:
        g, w = R.launches(got, name), R.launches(want, name)
        assert len(g) == len(w) > 20, (name, len(g), len(w))
        for i, (a, b) in enumerate(zip(g, w)):
            assert a == b, (name, i, {k: (a.get(k), b.get(k)) for k in set(a) | set(b) if a.get(k) != b.get(k)})
