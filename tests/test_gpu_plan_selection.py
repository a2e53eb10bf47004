"""Plan creation selects today what it selected when tests/golden/plan_selection.json was recorded: the characterisation of
the scheduler (hackathon_fft_amd/csrc/schedule.cpp) and of every dispatched route.  The file is the output of
tools/plan_snapshot.py on an MI355X at the commit before the general route moved out of mifft_plan_create_slab; a change
that alters selection on purpose regenerates it with the tool.  Plans only: nothing is executed and no data tensor allocated;
the two rebuild cases hold about 1 GB of plan scratch each while their plan lives."""
import json
import os

import pytest

from tools import plan_snapshot

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_selection.json")) as f:
    GOLDEN = json.load(f)


def test_the_fixture_and_the_tool_list_the_same_cases():
    assert list(GOLDEN) == list(plan_snapshot.CASES)


@pytest.mark.parametrize("case", list(plan_snapshot.CASES))
def test_plan_creation_selects_what_the_fixture_records(case):
    assert plan_snapshot.snapshot(case) == GOLDEN[case]


def test_a_slab_selects_as_its_whole_batch_does():
    names = lambda c: [d["kernel_name"] for d in plan_snapshot.snapshot(c)["dims"]]
    assert names("r_10x640x480_slab_of_100") == names("r_100x640x480")
