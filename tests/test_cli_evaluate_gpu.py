"""`mcq query -precision / -taxon-coverage` with MCQ_EVALUATE_DEVICE=1: the workers hand every batch's (assigned taxon, truth) pairs to
mc_evaluate_assignments instead of counting them, and the summary is printed from mc_evaluate_tally.

  * the golden cases `precision` and `precision_truth_lineage` (tests/golden/cli_expected.json.gz: the reference's own output) must come
    out line for line as without the switch, and MCQ_PROFILE must say how many calls and reads went through the library;
  * -taxon-coverage on tests/golden/evaluate_truth.fa, whose headers name taxa that toy32 does not cover.  The reference has no output
    to compare with: its -taxon-coverage ends in a segmentation fault (tests/golden/make_golden_evaluate.py says where).  The run with
    the switch must equal the run without it (mcq's host loop) line for line, and the whole summary -- the false-positive block, the
    only one of the four confusion counters that is printed, included -- must be what the model (tests/evaluate_ref.py) and
    api.Evaluation make of the run's own mapping lines.  The other three confusion counters are held to the model alone
    (tests/test_gpu_evaluate.py);
  * under -cov-percentile the host loop stays, and MCQ_PROFILE says so and why."""
import gzip
import json
import os
import re
import subprocess

import numpy as np
import pytest

import evaluate_ref
from metacache_amd import api, build

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


def cli_case(name):
    with gzip.open(os.path.join(GOLD, "cli_expected.json.gz"), "rt") as f:
        return json.load(f)[name]


def volatile(line):
    return re.match(r"^# (time:    |speed:   |Using \d+ threads$)", line) is not None


def same_lines(got, exp, tag):
    assert len(got) == len(exp), (tag, len(got), len(exp))
    for i, (g, e) in enumerate(zip(got, exp)):
        if volatile(e):
            assert volatile(g)
        else:
            assert g == e, (tag, i, g[:300], e[:300])


def run_mcq(files, args, out, device):
    build.build_library()
    env = dict(os.environ)
    env["MCQ_PROFILE"] = "1"
    env.pop("MCQ_EVALUATE_DEVICE", None)
    if device:
        env["MCQ_EVALUATE_DEVICE"] = "1"
    cmd = [build.MCQ, "query", "toy32"] + files + args + ["-threads", "1", "-out", str(out)]
    r = subprocess.run(cmd, cwd=GOLD, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr
    return out.read_text().split("\n"), r.stderr


def library_calls(stderr):
    m = re.search(r"evaluation on the device: (\d+) mc_evaluate_assignments calls, (\d+) reads, (\d+) batches counted on the host", stderr)
    assert m, stderr
    return tuple(int(x) for x in m.groups())


@pytest.mark.parametrize("case", ["precision", "precision_truth_lineage"])
def test_golden_precision_cases_through_the_library(case, tmp_path):
    c = cli_case(case)
    got, stderr = run_mcq(c["files"], c["args"], tmp_path / "out.txt", device=True)
    same_lines(got, c["lines"], case)
    calls, reads, on_host = library_calls(stderr)
    assert calls > 0 and reads == 300 and on_host == 0
    _, stderr = run_mcq(c["files"], c["args"], tmp_path / "out2.txt", device=False)      # without the switch: no word about it
    assert "evaluat" not in stderr


def test_taxon_coverage_equals_the_host_loop_and_the_model(tmp_path):
    args = ["-taxon-coverage", "-ground-truth", "-taxids"]
    got, stderr = run_mcq(["evaluate_truth.fa"], args, tmp_path / "dev.txt", device=True)
    host, _ = run_mcq(["evaluate_truth.fa"], args, tmp_path / "host.txt", device=False)
    same_lines(got, host, "taxon coverage: device against host")
    calls, reads, on_host = library_calls(stderr)
    assert calls > 0 and reads == 300 and on_host == 0
    # the model over the run's own mapping lines: query_header | truth | assigned, both as rank:name(taxid)
    db = api.Database.open(os.path.join(GOLD, "toy32"))
    try:
        taxa = db.taxa()
    finally:
        db.close()
    index_of_id = {t[0]: i for i, t in enumerate(taxa)}
    taxon = lambda col: 0 if col == "--" else index_of_id[int(re.fullmatch(r"\w+:.*\((-?\d+)\)", col).group(1))] + 1
    body = [l.split("\t|\t") for l in got if l and not l.startswith("#")]
    assert len(body) == 300
    truth = np.array([taxon(c[1]) for c in body], dtype=np.uint32)
    assigned = np.array([taxon(c[2]) for c in body], dtype=np.uint32)
    lin, rank, covered = evaluate_ref.taxon_table(taxa)
    _, want = evaluate_ref.evaluate(lin, rank, covered, assigned, truth, coverage=True)
    ev = api.Evaluation(want["assigned"], want["known"], want["correct"], want["wrong"], want["coverage"], want["reads"], want["out_of_table"])
    first = next(i for i, l in enumerate(got) if l.startswith("# unclassified:"))
    assert [l for l in got[first:] if l] == ev.summary_lines("# ")
    # what makes this file worth its bytes: false positives on some rank, and a truth that moved from a taxon without a rank to a ranked ancestor
    block = got.index("# false positives (hit on taxa not covered in DB):")
    assert any(int(l.split()[-1]) > 0 for l in got[block + 1:] if l)
    named = {h.split()[0]: int(h.split("|")[1]) for h in (l[1:] for l in open(os.path.join(GOLD, "evaluate_truth.fa")) if l.startswith(">e"))}
    rank_of_id = {t[0]: t[2] for t in taxa}
    moved = [c for c in body if c[0] in named and rank_of_id[named[c[0]]] == 21 and c[1] != "--" and taxa[taxon(c[1]) - 1][0] != named[c[0]]]
    assert moved and all(taxa[taxon(c[1]) - 1][2] < 21 for c in moved)


def test_cov_percentile_keeps_the_host_loop_and_says_so(tmp_path):
    _, stderr = run_mcq(["cli_truth.fa"], ["-precision", "-cov-percentile", "0.3"], tmp_path / "out.txt", device=True)
    assert "-precision: evaluated on the host (-cov-percentile" in stderr and "evaluation on the device" not in stderr
