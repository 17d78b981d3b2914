"""`mcq query` with MCQ_PARSE_DEVICE=1: a batch's reads are cut out of the file's bytes on the device (mc_batch_add_file_bytes) instead of
record by record on the worker thread.  The cases and the environment are those of test_cli_streaming_index_same_output -- 4 worker
threads, batches of 23 queries, the streaming index in chunks of 3 000 bytes -- plus the switch and MCQ_PROFILE: the output must be the
reference's, and the profile must say what the device took and what it left to the host, and why."""
import functools
import os
import re
import subprocess
import tempfile

import pytest

import parse_cases
import parse_ref
from metacache_amd import build
from test_cli_gpu import CASES, GOLD, _volatile

pytestmark = pytest.mark.gpu

ON_DEVICE = re.compile(r"mcq profile: reads parsed on the device: (\d+) batches, (\d+) bytes, (\d+) records, (\d+) batches parsed on the host(?: \((.*)\))?")
ON_HOST = re.compile(r"mcq: reads parsed on the host \((.*)\)")
OTHER_SWITCHES = {"MCQ_FORMAT_DEVICE": "1", "MCQ_EVALUATE_DEVICE": "1", "MCQ_TARGET_HITS_DEVICE": "1"}


@functools.lru_cache(maxsize=None)
def run(case, switched=True, others=False, extra=()):
    """one run of `mcq` (made once, shared by the tests) -> (lines without the volatile ones, stderr)"""
    build.build_library()
    c = CASES[case]
    env = {k: v for k, v in os.environ.items() if k != "MCQ_PARSE_DEVICE" and k not in OTHER_SWITCHES}
    env.update(MCQ_STREAM_MIN="0", MCQ_STREAM_CHUNK="3000", MCQ_PROFILE="1")
    if switched:
        env["MCQ_PARSE_DEVICE"] = "1"
    if others:
        env.update(OTHER_SWITCHES)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.txt")
        cmd = [build.MCQ, "query", "toy32"] + c["files"] + c["args"] + list(extra) + ["-threads", "4", "-out", out]
        if "-batch-size" not in c["args"]:
            cmd += ["-batch-size", "23"]
        r = subprocess.run(cmd, cwd=GOLD, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stderr
        with open(out) as f:
            return tuple(l for l in f.read().split("\n") if not _volatile(l) and "threads" not in l), r.stderr


def expected(case):
    return tuple(l for l in CASES[case]["lines"] if not _volatile(l) and "threads" not in l)


def records_of(case):
    return sum(len(parse_ref.parse(parse_cases.golden_bytes(f)).records) for f in CASES[case]["files"])


@pytest.mark.parametrize("case", ["everything_species", "pairseq", "two_files", "ground_truth"])
def test_regular_files_are_parsed_on_the_device(case):
    lines, stderr = run(case)
    assert lines == expected(case)
    m = ON_DEVICE.search(stderr)
    assert m, stderr
    batches, nbytes, records, host = (int(m.group(k)) for k in range(1, 5))
    assert host == 0 and m.group(5) is None, stderr
    assert records == records_of(case) and nbytes == sum(len(parse_cases.golden_bytes(f)) for f in CASES[case]["files"])
    assert batches >= records // (46 if "-pairseq" in CASES[case]["args"] else 23)


@pytest.mark.parametrize("case", ["fastq_irregular", "fastq_irregular_pairseq", "fasta_plus_lines", "irregular_with_regular"])
def test_irregular_files_keep_their_lines_and_say_what_stayed_on_the_host(case):
    lines, stderr = run(case)
    assert lines == expected(case)
    m = ON_DEVICE.search(stderr)
    assert m, stderr
    host = int(m.group(4))
    assert host > 0 and m.group(5), stderr                        # the batches of the exact reader, and the first one's reason
    assert "exact reader" in m.group(5) or "irregular at byte" in m.group(5) or "records" in m.group(5), stderr
    if case == "irregular_with_regular":                          # cli_pairs.fq between the two irregular files is regular: its batches go to the device
        assert int(m.group(3)) >= 240, stderr


@pytest.mark.parametrize("case,reason", [("gzip_input", "gzip"), ("pairfiles", "-pairfiles")])
def test_runs_that_stay_on_the_host_say_so(case, reason):
    lines, stderr = run(case)
    assert lines == expected(case)
    m = ON_HOST.search(stderr)
    assert m and reason in m.group(1) and not ON_DEVICE.search(stderr), stderr


def test_with_the_other_switches(tmp_path):
    lines, stderr = run("pairseq", others=True)
    assert lines == expected("pairseq")
    m = ON_DEVICE.search(stderr)
    assert m and int(m.group(4)) == 0 and int(m.group(3)) == 240, stderr
    assert "mapping lines on the device" in stderr


def test_without_the_switch_nothing_changes():
    lines, stderr = run("everything_species", switched=False)
    assert lines == expected("everything_species")
    assert "parsed on" not in stderr
    lines, stderr = run("gzip_input", switched=False)
    assert lines == expected("gzip_input") and "parsed on" not in stderr
