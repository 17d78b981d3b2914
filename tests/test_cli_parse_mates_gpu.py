"""`mcq query -pairfiles` with MCQ_PARSE_DEVICE=2: a batch's pairs are cut out of the two files' bytes on the device
(mc_batch_add_file_mates).  Every case of test_cli_gpu.CASES that holds -pairfiles runs in the environment of test_cli_parse_gpu.run
with the switch at 2: the lines must be the golden ones, and the profile must say that no batch was left to the host and count the
records and bytes of both files.  With the switch at 1 the same cases stay on the host and say why, as before."""
import functools
import os
import subprocess
import tempfile

import pytest

import parse_cases
import parse_ref
from metacache_amd import build
from test_cli_gpu import CASES, GOLD, _volatile
from test_cli_parse_gpu import ON_DEVICE, ON_HOST, OTHER_SWITCHES

pytestmark = pytest.mark.gpu
PAIRFILES = sorted(c for c in CASES if isinstance(CASES[c], dict) and "-pairfiles" in CASES[c].get("args", ()))


@functools.lru_cache(maxsize=None)
def run(case, switch):
    """one run of `mcq` (made once) -> (output lines by file suffix; "" for -out, stderr)"""
    build.build_library()
    c = CASES[case]
    env = {k: v for k, v in os.environ.items() if k != "MCQ_PARSE_DEVICE" and k not in OTHER_SWITCHES}
    env.update(MCQ_STREAM_MIN="0", MCQ_STREAM_CHUNK="3000", MCQ_PROFILE="1", MCQ_PARSE_DEVICE=switch)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out")
        cmd = [build.MCQ, "query", "toy32"] + c["files"] + c["args"] + ["-threads", "4", "-split-out" if "split" in c else "-out", out]
        if "-batch-size" not in c["args"]:
            cmd += ["-batch-size", "23"]
        r = subprocess.run(cmd, cwd=GOLD, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stderr
        got = {}
        for f in sorted(os.listdir(tmp)):
            with open(os.path.join(tmp, f)) as fh:
                got[f[len("out"):]] = tuple(fh.read().split("\n"))
        return got, r.stderr


def assert_golden_lines(case, got):
    """the lines of every output file are the golden ones (the volatile lines aside, as test_cli_parse_gpu compares them)"""
    keep = lambda lines: tuple(l for l in lines if not _volatile(l) and "threads" not in l)
    c = CASES[case]
    want = c["split"] if "split" in c else {"": c["lines"]}
    assert sorted(got) == sorted(want)
    for suffix, exp in want.items():
        assert keep(got[suffix]) == keep(exp), (case, suffix)


def test_there_are_pairfiles_cases():
    assert "pairfiles" in PAIRFILES


@pytest.mark.parametrize("case", PAIRFILES)
def test_pairfiles_batches_are_parsed_on_the_device(case):
    got, stderr = run(case, "2")
    assert_golden_lines(case, got)
    m = ON_DEVICE.search(stderr)
    assert m, stderr
    batches, nbytes, records, host = (int(m.group(k)) for k in range(1, 5))
    assert host == 0 and m.group(5) is None, stderr
    files = CASES[case]["files"]
    per_file = [len(parse_ref.parse(parse_cases.golden_bytes(f)).records) for f in files]
    assert per_file[0::2] == per_file[1::2]                       # (equal counts: whole files go to the device)
    assert records == sum(per_file) and nbytes == sum(len(parse_cases.golden_bytes(f)) for f in files)
    assert batches >= 1


@pytest.mark.parametrize("case", PAIRFILES)
def test_with_the_switch_at_1_pairfiles_stay_on_the_host(case):
    got, stderr = run(case, "1")
    assert_golden_lines(case, got)
    m = ON_HOST.search(stderr)
    assert m and "-pairfiles" in m.group(1) and not ON_DEVICE.search(stderr), stderr
