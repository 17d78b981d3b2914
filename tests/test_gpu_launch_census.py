"""GPU: the per-batch pipeline launches what it launched at the commit tests/golden/launch_census.json was recorded from -- per case and
batch the count of every timed step (tools/launch_census.py: the synchronous call, taxon key, deferred tail, the four wants, the lane
path's switches, the 8-byte store, the lookups inside the filter kernel, the slot path with and without a long read, the owner side of
Mode K), zero counts included.  What the steps compute is the other GPU tests' business."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import launch_census  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def census():
    return launch_census.run()


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "launch_census.json")) as f:
        return json.load(f)


def test_recorded_census_names_every_case_and_timer(recorded):
    assert sorted(recorded["cases"]) == sorted(launch_census.CASES) and recorded["skipped"] == []
    assert recorded["timers"] == list(launch_census.TIMERS) and len(recorded["commit"]) >= 7
    for case, batches in recorded["cases"].items():
        for batch, counts in batches.items():
            assert sorted(counts) == sorted(launch_census.TIMERS), (case, batch)
            assert sum(counts.values()) > 0, (case, batch)


@pytest.mark.parametrize("case", launch_census.CASES)
def test_every_timed_step_runs_as_often_as_recorded(census, recorded, case):
    if case in census["skipped"]:
        assert case in launch_census.SKIPPABLE, case
        pytest.skip("the device had no room for the direct index")
    got, want = census["cases"][case], recorded["cases"][case]
    assert sorted(got) == sorted(want), case
    for batch in want:
        for name in launch_census.TIMERS:
            assert got[batch][name] == want[batch][name], (case, batch, name, got[batch], want[batch])
