"""`mcq merge` on the generated part files (golden/merge_cases_in) against the reference's `metacache merge`
(merge_cases_expected.json.gz), by the host path; and the switch MCQ_MERGE_DEVICE=1: whether a device is there or not the lines are the
same and stderr says under MCQ_PROFILE who merged -- the fall-back is never silent.  Runs without a GPU."""
import gzip
import json
import os
import subprocess

import pytest

from metacache_amd import build
from test_cli_gpu import _same

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
DEVICE_LINE = "mcq profile: result files merged on the device: "
HOST_LINE = "mcq: result files merged on the host ("

with gzip.open(os.path.join(GOLD, "merge_cases_expected.json.gz"), "rt") as f:
    EXP = json.load(f)


def run_merge(c, out, env=None):
    build.build_library()
    e = dict(os.environ)
    e.pop("MCQ_MERGE_DEVICE", None)
    e.pop("MCQ_PROFILE", None)
    e.update(env or {})
    r = subprocess.run([build.MCQ, "merge"] + c["files"] + ["-taxonomy", "build_in/taxonomy"] + c["args"] + ["-out", str(out)], cwd=GOLD,
                       capture_output=True, text=True, timeout=300, env=e)
    assert r.returncode == 0, r.stderr
    return out.read_text().split("\n"), r.stderr


@pytest.mark.parametrize("case", sorted(EXP))
def test_host_merge_matches_reference(case, tmp_path):
    got, err = run_merge(EXP[case], tmp_path / "merged.txt", {"MCQ_PROFILE": "1"})
    _same(got, EXP[case]["lines"], case)
    assert DEVICE_LINE not in err and HOST_LINE not in err              # the switch is unset: no word about it


def test_switch_never_falls_back_silently(tmp_path):
    c = EXP["three_maxcand8"]
    got, err = run_merge(c, tmp_path / "merged.txt", {"MCQ_MERGE_DEVICE": "1", "MCQ_PROFILE": "1"})
    _same(got, c["lines"], "three_maxcand8")
    assert (DEVICE_LINE in err and "0 files left to the host" in err) != (HOST_LINE in err), err
    # without MCQ_PROFILE a merge on the device says nothing, a fall-back is still named
    fell_back = HOST_LINE in err
    got, err = run_merge(c, tmp_path / "plain.txt", {"MCQ_MERGE_DEVICE": "1"})
    _same(got, c["lines"], "three_maxcand8")
    assert DEVICE_LINE not in err and (HOST_LINE in err) == fell_back, err
