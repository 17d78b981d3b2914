"""GPU: `mcq merge` with MCQ_MERGE_DEVICE=1 (mc_merge_results_*) on every case of merge_expected.json.gz and of
merge_cases_expected.json.gz: the lines are the reference's, stderr holds the profile line with "0 files left to the host".  A part file
made irregular (a '\\r\\n' line) leaves the merge to the host: the same lines as the host path prints for that input, the file and the
offence named on stderr.  With the switch unset stderr holds no such line."""
import gzip
import json
import os
import shutil
import subprocess

import pytest

from metacache_amd import build
from test_cli_gpu import _same

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
DEVICE_LINE = "mcq profile: result files merged on the device: "
HOST_LINE = "mcq: result files merged on the host ("

EXP = {}
for name in ("merge_expected.json.gz", "merge_cases_expected.json.gz"):
    with gzip.open(os.path.join(GOLD, name), "rt") as f:
        EXP.update(json.load(f))


def run_merge(files, args, out, device=True, profile=True):
    build.build_library()
    env = dict(os.environ)
    env.pop("MCQ_MERGE_DEVICE", None)
    env.pop("MCQ_PROFILE", None)
    if profile:
        env["MCQ_PROFILE"] = "1"
    if device:
        env["MCQ_MERGE_DEVICE"] = "1"
    r = subprocess.run([build.MCQ, "merge"] + files + ["-taxonomy", "build_in/taxonomy"] + args + ["-out", str(out)], cwd=GOLD,
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr
    return out.read_text().split("\n"), r.stderr


@pytest.mark.parametrize("case", sorted(EXP))
def test_device_merge_matches_reference(case, tmp_path):
    c = EXP[case]
    files = c["files"]
    if case == "directory":
        d = tmp_path / "merge_dir"
        d.mkdir()
        for part in (0, 1):
            os.symlink(os.path.join(GOLD, f"merge_in/part{part}.txt"), d / f"part{part}.txt")
        files = [str(d)]
    got, err = run_merge(files, c["args"], tmp_path / "merged.txt")
    exp = c["lines"]
    if case == "directory":                       # the file names are part of the output
        got = [l for l in got if "part" not in l or not l.startswith("# ")]
        exp = [l for l in exp if "part" not in l or not l.startswith("# ")]
    _same(got, exp, case)
    line = next((l for l in err.split("\n") if l.startswith(DEVICE_LINE)), None)
    assert line and line.endswith("0 files left to the host") and f"{len(c['files']) if case != 'directory' else 2} files" in line, err
    assert HOST_LINE not in err


def test_irregular_file_goes_to_the_host_and_says_so(tmp_path):
    c = EXP["three_maxcand8"]
    d = tmp_path / "merge_cases_in"
    shutil.copytree(os.path.join(GOLD, "merge_cases_in"), d)
    data = (d / "b.txt").read_bytes()
    at = data.index(b"\n12\t|") + 1                               # the line of id 12 gets a '\r\n' end
    end = data.index(b"\n", at)
    (d / "b.txt").write_bytes(data[:end] + b"\r" + data[end:])
    files = [str(d / "a.txt"), str(d / "b.txt"), str(d / "c.txt")]
    host, err_host = run_merge(files, c["args"], tmp_path / "host.txt", device=False)
    dev, err = run_merge(files, c["args"], tmp_path / "dev.txt")
    _same(dev, host, "irregular b.txt")                         # (but for the time and speed lines)
    assert DEVICE_LINE not in err_host and HOST_LINE not in err_host
    line = next((l for l in err.split("\n") if l.startswith(HOST_LINE)), None)
    assert line and str(d / "b.txt") in line and f"irregular line at offset {at}" in line and DEVICE_LINE not in err, err
    # the switch was set: the fall-back is named without MCQ_PROFILE too, unless the run is -silent
    plain, err = run_merge(files, c["args"], tmp_path / "plain.txt", profile=False)
    _same(plain, host, "irregular b.txt, no profile")
    assert line in err.split("\n")
    quiet, err = run_merge(files, c["args"] + ["-silent"], tmp_path / "quiet.txt", profile=False)
    _same(quiet, host, "irregular b.txt, silent")
    assert HOST_LINE not in err and DEVICE_LINE not in err


def test_switch_unset_says_nothing(tmp_path):
    c = EXP["default"]
    got, err = run_merge(c["files"], c["args"], tmp_path / "merged.txt", device=False)
    _same(got, c["lines"], "default")
    assert DEVICE_LINE not in err and HOST_LINE not in err
