"""`mcq query -hits-per-ref` builds its lists with the library (mc_target_hits_add per batch, mc_target_hits_collect at the end): the lines
are the reference's, compared as test_cli_gpu.py compares them, and the run says under MCQ_PROFILE that the device path was taken."""
import os
import re
import subprocess

import pytest

from metacache_amd import build
from test_cli_gpu import CASES, GOLD, _same

pytestmark = pytest.mark.gpu

STATS = re.compile(r"mcq profile: hits per target on the device: (\d+) mc_target_hits_add calls, (\d+) records, (\d+) targets, (\d+) records of (\d+) batches kept on the host")


def run(case, tmp_path, args, threads="1", host_every=0):
    build.build_library()
    c = CASES[case]
    out = tmp_path / "out.txt"
    cmd = [build.MCQ, "query", "toy32"] + c["files"] + args + ["-threads", threads, "-out", str(out)]
    r = subprocess.run(cmd, cwd=GOLD, capture_output=True, text=True, timeout=600, env=dict(os.environ, MCQ_PROFILE="1", MCQ_TARGET_HITS_DEVICE="1", MCQ_TARGET_HITS_HOST_EVERY=str(host_every)))
    assert r.returncode == 0, r.stderr
    assert "lists built on the host" not in r.stderr, r.stderr
    m = STATS.search(r.stderr)
    assert m, r.stderr
    calls, records, targets, host_records, host_batches = map(int, m.groups())
    assert calls > 0 and records > 0 and targets > 0
    if host_every:
        assert host_records > 0 and host_batches > 0 and "MCQ_TARGET_HITS_HOST_EVERY" in r.stderr
    else:
        assert host_records == 0 and host_batches == 0
    return out.read_text().split("\n"), records + host_records


def listed_records(lines):
    """the entries of the per-target lines: <sequence> TAB <windows> TAB <query>/<window>+<more>:<hits>,..."""
    return sum(len(l.split("\t")[-1].split(",")) for l in lines if re.search(r"\t\d+/\d+\+\d+:\d+(,|$)", l))


@pytest.mark.parametrize("case", ["hits_per_ref", "hits_per_ref_lineage"])
def test_lists_from_the_device_equal_the_reference(case, tmp_path):
    c = CASES[case]
    got, records = run(case, tmp_path, c["args"])
    _same(got, c["lines"], case, unordered=True)
    assert listed_records(got) == records                                 # every record the library counted is on a line


def test_lists_in_a_file_of_their_own(tmp_path):
    case = "analysis_files"
    c = CASES[case]
    extra = {k: str(tmp_path / (case + "." + k)) for k in c["extra"]}
    got, records = run(case, tmp_path, [a.format(**extra) for a in c["args"]])
    _same(got, c["main"], (case, "main"))
    for k, exp in c["extra"].items():
        _same(open(extra[k]).read().split("\n"), exp, (case, k), unordered=(k == "targets"))
    assert listed_records(open(extra["targets"]).read().split("\n")) == records


@pytest.mark.parametrize("threads", ["1", "4"])
def test_batches_that_stay_on_the_host_are_merged_in(tmp_path, threads):
    """every second batch of a worker is kept on the host as if its mc_target_hits_add had failed: the lines are the same, made of
    the device's records and the host's"""
    c = CASES["hits_per_ref"]
    got, records = run("hits_per_ref", tmp_path, c["args"] + ["-batch-size", "23"], threads=threads, host_every=2)
    exp = [l for l in c["lines"] if "threads" not in l]
    got = [l for l in got if "threads" not in l]
    _same(got, exp, ("hits_per_ref", "host_every", threads), unordered=True)
    assert listed_records(got) == records
