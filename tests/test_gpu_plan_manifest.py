"""GPU: the plan builder (csrc/engine.hip build_graph) still produces, case by case, what tests/golden/plan_manifest.json recorded: the
same launches in the same order with the same flops / bytes figures, the same arena size (so the same allocation order), the same number
of hipGraph nodes, and - no kernel having changed - the same result block bit for bit.  A matching op list with another result hash means
that a launch ARGUMENT changed.  The fixture is regenerated (tools/plan_manifest.py --out ...) only by a change that means to alter a plan."""
import json
import os

import pytest

from tests.util import GOLDEN_DIR
from tools import plan_manifest

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN_DIR, "plan_manifest.json")) as _f:
    RECORDED = json.load(_f)
CASES = plan_manifest.cases()


def test_the_fixture_holds_exactly_the_cases_of_the_tool():
    assert sorted(RECORDED) == sorted(c[0] for c in CASES)


def test_the_r50_default_case_reaches_the_stem_and_average_fusions():
    names = [op[0] for op in RECORDED[f"r50-{plan_manifest.R50_SIZE[0]}x{plan_manifest.R50_SIZE[1]}-bs1-f16x3"]["ops"]]
    assert "backbone.stem.2+pool" in names and "backbone.s1.b0.avgpool" not in names


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_plan_equals_the_recorded_manifest(case):
    want, got = RECORDED[case[0]], plan_manifest.record(case)
    diff = plan_manifest.first_difference(want, got)
    print(case[0], len(got["ops"]), "ops", got["arena_bytes"], "arena bytes", got["graph_nodes"], "graph nodes", got["result_sha256"][:16], diff or "equal")
    assert not diff, f"{case[0]}: {diff}"
    assert got == want
