"""`mcq query` with MCQ_INFLATE_DEVICE=1: a BGZF query file is indexed on the host (mc_bgzf_index) and inflated on the device
(mc_inflate_blocks) instead of through gzread.  BGZF files of the golden reads are written into a temporary directory under the names the
golden cases use, so the output must be the reference's line for line; the profile must say what the device took, and which file it
left to the host and why.  A file the device refuses must come out exactly as without the switch."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import inflate_cases
from metacache_amd import build
from test_cli_gpu import CASES, GOLD, _volatile

pytestmark = pytest.mark.gpu

ON_DEVICE = re.compile(r"mcq profile: gzip input inflated on the device: (\d+) files, (\d+) blocks, (\d+) bytes in, (\d+) bytes out, (\d+) files left to the host(?: \((.*)\))?")
SWITCHES = ("MCQ_INFLATE_DEVICE", "MCQ_FORMAT_DEVICE", "MCQ_EVALUATE_DEVICE", "MCQ_PARSE_DEVICE", "MCQ_TARGET_HITS_DEVICE")
PAYLOAD = 3000           # many members per file


def golden(name):
    with open(os.path.join(GOLD, name), "rb") as f:
        return f.read()


def bgzf(name):
    return inflate_cases.bgzf_file(golden(name), payload=PAYLOAD)


def flipped(data):
    """one payload byte of the third member flipped"""
    import inflate_ref
    rows = inflate_ref.walk(data)[0]
    bad = bytearray(data)
    bad[rows[2][0] + 18 + 40] ^= 0x10
    return bytes(bad)


@functools.lru_cache(maxsize=None)
def run(case, kind, switched=True, others=False):
    """one run of `mcq` on the case's files as `kind` (bgzf / flipped / golden: the committed files) -> (lines, stderr, return code)"""
    build.build_library()
    c = CASES[case]
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env["MCQ_PROFILE"] = "1"
    if switched:
        env["MCQ_INFLATE_DEVICE"] = "1"
    if others:
        env.update(MCQ_FORMAT_DEVICE="1", MCQ_EVALUATE_DEVICE="1", MCQ_PARSE_DEVICE="1")
    with tempfile.TemporaryDirectory() as tmp:
        for f in c["files"]:
            if kind == "golden":
                shutil.copy(os.path.join(GOLD, f), os.path.join(tmp, f))
                continue
            data = bgzf(f[:-3] if f.endswith(".gz") else f)
            with open(os.path.join(tmp, f), "wb") as o:
                o.write(flipped(data) if kind == "flipped" else data)
        out = os.path.join(tmp, "out.txt")
        cmd = [build.MCQ, "query", os.path.join(GOLD, "toy32")] + c["files"] + c["args"] + ["-threads", "4", "-batch-size", "23", "-out", out]
        r = subprocess.run(cmd, cwd=tmp, capture_output=True, text=True, timeout=600, env=env)
        lines = ()
        if os.path.exists(out):
            with open(out) as f:
                lines = tuple(l for l in f.read().split("\n") if not _volatile(l) and "threads" not in l)
        return lines, r.stderr, r.returncode


def expected(case):
    return tuple(l for l in CASES[case]["lines"] if not _volatile(l) and "threads" not in l)


@pytest.mark.parametrize("case", ["gzip_input", "pairfiles"])
def test_bgzf_files_are_inflated_on_the_device(case):
    lines, stderr, rc = run(case, "bgzf")
    assert rc == 0, stderr
    assert lines == expected(case)
    m = ON_DEVICE.search(stderr)
    assert m, stderr
    files, blocks, bytes_in, bytes_out, host = (int(m.group(k)) for k in range(1, 6))
    names = [f[:-3] if f.endswith(".gz") else f for f in CASES[case]["files"]]
    assert host == 0 and m.group(6) is None, stderr
    assert files == len(names) and bytes_out == sum(len(golden(n)) for n in names) and bytes_in == sum(len(bgzf(n)) for n in names)
    assert blocks == sum((len(golden(n)) + PAYLOAD - 1) // PAYLOAD + 1 for n in names) and blocks > 2 * files


def test_plain_gzip_goes_to_the_host_and_says_so():
    lines, stderr, rc = run("gzip_input", "golden")
    assert rc == 0 and lines == expected("gzip_input")
    m = ON_DEVICE.search(stderr)
    assert m and [int(m.group(k)) for k in range(1, 6)] == [0, 0, 0, 0, 1], stderr
    assert "cli_reads.fa.gz: not BGZF" in m.group(6)


def test_a_refused_file_comes_out_as_without_the_switch():
    lines, stderr, rc = run("gzip_input", "flipped")
    plain_lines, plain_stderr, plain_rc = run("gzip_input", "flipped", switched=False)
    assert (lines, rc) == (plain_lines, plain_rc)
    m = ON_DEVICE.search(stderr)
    assert m and [int(m.group(k)) for k in range(1, 6)] == [0, 0, 0, 0, 1] and "the device refused block 2" in m.group(6), stderr
    cut = lambda s: s[:s.index("mcq profile:")] if "mcq profile:" in s else s
    assert cut(stderr) == cut(plain_stderr)
    assert "inflated on" not in plain_stderr


def test_without_the_switch_nothing_changes():
    for kind in ("bgzf", "golden"):
        lines, stderr, rc = run("gzip_input", kind, switched=False)
        assert rc == 0 and lines == expected("gzip_input") and "inflated on" not in stderr


def test_with_the_other_switches():
    lines, stderr, rc = run("gzip_input", "bgzf", others=True)
    assert rc == 0 and lines == expected("gzip_input")
    m = ON_DEVICE.search(stderr)
    assert m and int(m.group(5)) == 0 and int(m.group(1)) == 1, stderr
    assert "reads parsed on the host (gzip input" in stderr          # inflated input still does not take the device parse
