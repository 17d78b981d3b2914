"""`mcq query` with its device hand-offs switched on TOGETHER: MCQ_FORMAT_DEVICE=1 (the mapping lines), MCQ_EVALUATE_DEVICE=1 (-precision)
and MCQ_TARGET_HITS_DEVICE=1 (-hits-per-ref).  With the first one set, the worker that takes a batch's lines from the library is also the one
that fills the other two hand-offs' buffers, so the three are checked in one run here; the tests of each switch alone are
test_cli_format_gpu.py, test_cli_evaluate_gpu.py and test_cli_target_hits_gpu.py.

  * three command lines -- the golden cases `precision` and `hits_per_ref_lineage`, and `precision` with `-hits-per-ref -tophits -queryids`
    appended (the one that engages all three hand-offs) -- give, with the switches set, the lines of the same command without them; the
    first two give their goldens as well; every hand-off the command engages says under MCQ_PROFILE that it ran on the device and kept no
    batch on the host, and the evaluation saw as many reads as the formatter;
  * the third command again with MCQ_TARGET_HITS_HOST_EVERY=2 (and -batch-size 23, so that a worker has a second batch to keep): same
    lines, batches of the hits hand-off on the host, none of the other two;
  * -cov-percentile keeps all three on the host: the golden comes out, each hand-off says so and why, and the coverage step counts on the
    device."""
import functools
import os
import re
import subprocess
import tempfile

import pytest

from metacache_amd import build
from test_cli_format_gpu import GOLD, cli_case, same_lines

pytestmark = pytest.mark.gpu

SWITCHES = {"MCQ_FORMAT_DEVICE": "1", "MCQ_EVALUATE_DEVICE": "1", "MCQ_TARGET_HITS_DEVICE": "1"}
FORMAT = re.compile(r"mcq profile: mapping lines on the device: (\d+) mc_format_mappings calls, (\d+) reads, (\d+) lines, (\d+) batches formatted on the host")
EVALUATE = re.compile(r"mcq profile: evaluation on the device: (\d+) mc_evaluate_assignments calls, (\d+) reads, (\d+) batches counted on the host")
HITS = re.compile(r"mcq profile: hits per target on the device: (\d+) mc_target_hits_add calls, (\d+) records, (\d+) targets, (\d+) records of (\d+) batches kept on the host")
ON_HOST = {"format": re.compile(r"mcq: mapping lines formatted on the host \((.*)\)"),
           "evaluate": re.compile(r"mcq: -precision: evaluated on the host \((.*)\)"),
           "hits": re.compile(r"mcq: -hits-per-ref: lists built on the host \((.*)\)")}
COVERAGE = re.compile(r"mcq profile: coverage on the device: (\d+) mc_coverage_add calls, (\d+) candidates marked, (\d+) windows covered")

ALL_THREE = ["-hits-per-ref", "-tophits", "-queryids"]


def command(name):
    """-> (files, args, golden lines or None)"""
    if name == "precision_all_three":
        c = cli_case("precision")
        return c["files"], c["args"] + ALL_THREE, None
    if name == "cov_percentile_all_three":
        c = cli_case("cov_percentile_pct_hits_per_ref")
        return c["files"], c["args"] + ["-precision"], None
    c = cli_case(name)
    return c["files"], c["args"], c["lines"]


@functools.lru_cache(maxsize=None)
def run(name, switched, host_every=0, extra=()):
    """one run of `mcq` (made once, shared by the tests) -> (lines, stderr)"""
    build.build_library()
    files, args, _ = command(name)
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES and k != "MCQ_TARGET_HITS_HOST_EVERY"}
    env["MCQ_PROFILE"] = "1"
    if switched:
        env.update(SWITCHES)
    if host_every:
        env["MCQ_TARGET_HITS_HOST_EVERY"] = str(host_every)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.txt")
        cmd = [build.MCQ, "query", "toy32"] + files + args + list(extra) + ["-threads", "1", "-out", out]
        r = subprocess.run(cmd, cwd=GOLD, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stderr
        with open(out) as f:
            return tuple(f.read().split("\n")), r.stderr


def engaged(args):
    return {"format": True, "evaluate": "-precision" in args, "hits": "-hits-per-ref" in args}


def reports(stderr):
    """-> {hand-off: its counts} for the "on the device" lines of a run's stderr"""
    found = {}
    for key, rx in (("format", FORMAT), ("evaluate", EVALUATE), ("hits", HITS)):
        m = rx.findall(stderr)
        assert len(m) <= 1, stderr
        if m:
            found[key] = tuple(int(x) for x in m[0])
    return found


@pytest.mark.parametrize("name", ["precision", "hits_per_ref_lineage", "precision_all_three"])
def test_the_switches_together_change_no_line(name):
    files, args, golden = command(name)
    unordered = "-hits-per-ref" in args
    got, stderr = run(name, True)
    plain, plain_stderr = run(name, False)
    same_lines(list(got), list(plain), (name, "switched against plain"), lists_unordered=unordered)
    if golden is not None:
        same_lines(list(got), golden, (name, "golden"), lists_unordered=unordered)
    want = engaged(args)
    if name == "precision_all_three":
        assert all(want.values())
    rep = reports(stderr)
    assert set(rep) == {k for k, v in want.items() if v}, stderr
    for key, rx in ON_HOST.items():
        assert not rx.search(stderr), (key, stderr)
    calls, reads, lines, on_host = rep["format"]
    assert calls > 0 and reads > 0 and lines > 0 and on_host == 0, stderr
    if want["evaluate"]:
        ecalls, ereads, ehost = rep["evaluate"]
        assert ecalls > 0 and ehost == 0 and ereads == reads, stderr
    if want["hits"]:
        hcalls, records, targets, host_records, host_batches = rep["hits"]
        assert hcalls > 0 and records > 0 and targets > 0 and host_records == 0 and host_batches == 0, stderr
    # without the switches: no word about the library's lines or counts, and -hits-per-ref says that the host sort is the default
    assert not reports(plain_stderr) and not ON_HOST["format"].search(plain_stderr) and not ON_HOST["evaluate"].search(plain_stderr), plain_stderr


def test_hits_batches_kept_on_the_host_leave_the_other_two_alone():
    name = "precision_all_three"
    got, stderr = run(name, True, host_every=2, extra=("-batch-size", "23"))
    plain, _ = run(name, False)
    same_lines(list(got), list(plain), (name, "host_every"), lists_unordered=True)
    rep = reports(stderr)
    assert set(rep) == {"format", "evaluate", "hits"}, stderr
    hcalls, records, targets, host_records, host_batches = rep["hits"]
    assert hcalls > 0 and records > 0 and host_records > 0 and host_batches > 0 and "(MCQ_TARGET_HITS_HOST_EVERY)" in stderr, stderr
    calls, reads, lines, on_host = rep["format"]
    ecalls, ereads, ehost = rep["evaluate"]
    assert calls > 1 and on_host == 0 and ecalls == calls and ehost == 0 and ereads == reads, stderr


@pytest.mark.parametrize("name", ["cov_percentile_pct_hits_per_ref", "cov_percentile_all_three"])
def test_cov_percentile_keeps_all_three_on_the_host_and_says_so(name):
    files, args, golden = command(name)
    got, stderr = run(name, True)
    if golden is not None:
        same_lines(list(got), golden, (name, "golden"), lists_unordered=True)
    else:
        same_lines(list(got), list(run(name, False)[0]), (name, "switched against plain"), lists_unordered=True)
        assert all(engaged(args).values())
    assert not reports(stderr), stderr
    for key, wanted in engaged(args).items():
        m = ON_HOST[key].search(stderr)
        assert (m is not None) == wanted, (key, stderr)
        if wanted:
            assert "-cov-percentile" in m.group(1), (key, stderr)
    m = COVERAGE.search(stderr)
    assert m and int(m.group(1)) > 0 and int(m.group(2)) > 0 and int(m.group(3)) > 0, stderr
    assert "covered windows counted on the host" not in stderr, stderr
