"""`mcq query -allhits` with MCQ_FORMAT_DEVICE=1 and MCQ_ALLHITS_DEVICE=1: a worker gathers a batch's location lists, has the library
render the all-hits column (mc_format_matches) and puts it into the lines (mc_format_mappings_with); the host loop (show_matches,
MappingWriter) is not run for those batches.

  * the four golden command lines with -allhits of tests/golden/cli_expected.json.gz (the reference's own output) must come out line
    for line, and MCQ_PROFILE must say that every read went through both calls and no batch stayed on the host;
  * MCQ_ALLHITS_DEVICE=1 alone changes nothing and says nothing (with MCQ_FORMAT_DEVICE=1 alone -allhits keeps the host loop:
    tests/test_cli_format_gpu.py)."""
import gzip
import json
import os
import re
import subprocess

import pytest

from metacache_amd import build

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
CASES = ["everything_species", "allhits_sequence", "pairfiles", "reference_test_matrix"]


def cli_case(name):
    with gzip.open(os.path.join(GOLD, "cli_expected.json.gz"), "rt") as f:
        return json.load(f)[name]


def volatile(line):
    return re.match(r"^(# |%%)(time:    |speed:   |Using \d+ threads$)", line) is not None


def same_lines(got, exp, tag):
    assert len(got) == len(exp), (tag, len(got), len(exp))
    for i, (g, e) in enumerate(zip(got, exp)):
        if volatile(e):
            assert volatile(g)
        else:
            assert g == e, (tag, i, g[:300], e[:300])


def run_mcq(files, args, out, switches):
    build.build_library()
    env = dict(os.environ, MCQ_PROFILE="1")
    for name in ("MCQ_FORMAT_DEVICE", "MCQ_ALLHITS_DEVICE"):
        env.pop(name, None)
    env.update(switches)
    cmd = [build.MCQ, "query", "toy32"] + files + args + ["-threads", "1", "-out", str(out)]
    r = subprocess.run(cmd, cwd=GOLD, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr
    return out.read_text().split("\n"), r.stderr


@pytest.mark.parametrize("case", CASES)
def test_golden_cases_with_the_all_hits_column_from_the_library(case, tmp_path):
    c = cli_case(case)
    assert "-allhits" in c["args"]
    got, stderr = run_mcq(c["files"], c["args"], tmp_path / "out.txt", {"MCQ_FORMAT_DEVICE": "1", "MCQ_ALLHITS_DEVICE": "1"})
    same_lines(got, c["lines"], case)
    lines = re.findall(r"mapping lines on the device: (\d+) mc_format_mappings calls, (\d+) reads, (\d+) lines, (\d+) batches formatted on the host", stderr)
    column = re.findall(r"all-hits columns on the device: (\d+) mc_format_matches calls, (\d+) reads, (\d+) bytes", stderr)
    assert len(lines) == 1 and len(column) == 1, stderr
    calls, reads, printed, on_host = (int(x) for x in lines[0])
    mcalls, mreads, mbytes = (int(x) for x in column[0])
    assert calls > 0 and on_host == 0 and "0 batches formatted on the host" in stderr
    assert mcalls == calls and mreads == reads > 0 and printed > 0
    # the bytes are the all-hits columns of the reference's lines: the column behind the name (and the truth)
    at = 1 + ("-queryids" in c["args"]) + ("-ground-truth" in c["args"])
    ncols = at + 3
    body = [l for l in c["lines"] if l and not l.startswith("# ")]
    mapping = body[:next((i for i, l in enumerate(body) if len(l.split("\t|\t")) != ncols), len(body))]
    assert printed == len(mapping) and mbytes == sum(len(l.split("\t|\t")[at]) for l in mapping) > 0
    assert "formatted on the host (" not in stderr


def test_the_all_hits_switch_alone_changes_nothing_and_says_nothing(tmp_path):
    c = cli_case("allhits_sequence")
    got, stderr = run_mcq(c["files"], c["args"], tmp_path / "out.txt", {"MCQ_ALLHITS_DEVICE": "1"})
    same_lines(got, c["lines"], "allhits_sequence")
    assert "mapping lines" not in stderr and "all-hits" not in stderr and "mc_format" not in stderr
