"""`mcq query` with MCQ_INPUT_DEVICE=1: a query file is made resident on the device (a plain file uploaded, a BGZF file inflated there), cut
into batches there (mc_parse_cut, in pieces of MCQ_INPUT_DEVICE_PIECE bytes chained by `consumed`) and fed to the slots as device
ranges (mc_batch_add_device_bytes); only headers and candidates come back.  The output must be the reference's line for line; the profile
must say what went resident, and name every file that was left to the host with its reason.  Files the path does not take come out
exactly as before."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import inflate_cases
import parse_ref
from metacache_amd import build
from test_cli_gpu import CASES, GOLD, _volatile

pytestmark = pytest.mark.gpu

RESIDENT = re.compile(r"mcq profile: input resident on the device: (\d+) files, (\d+) pieces, (\d+) batches, (\d+) bytes, (\d+) records, (\d+) files left to the host(?: \((.*)\))?")
SWITCHES = ("MCQ_INPUT_DEVICE", "MCQ_INPUT_DEVICE_PIECE", "MCQ_INPUT_DEVICE_MB", "MCQ_INFLATE_DEVICE", "MCQ_FORMAT_DEVICE", "MCQ_EVALUATE_DEVICE", "MCQ_PARSE_DEVICE",
            "MCQ_TARGET_HITS_DEVICE")
PIECE, PAYLOAD = 3000, 3000


def golden(name):
    with open(os.path.join(GOLD, name), "rb") as f:
        return f.read()


def plain_name(f):
    return f[:-3] if f.endswith(".gz") else f


def flipped(data):
    """one payload byte of the third member flipped"""
    import inflate_ref
    rows = inflate_ref.walk(data)[0]
    bad = bytearray(data)
    bad[rows[2][0] + 18 + 40] ^= 0x10
    return bytes(bad)


@functools.lru_cache(maxsize=None)
def run(case, kind="golden", switched=True, others=False, cap_mb=None):
    """one run of `mcq` on the case's files as `kind` (golden: the committed files; bgzf / flipped: BGZF files of their plain bytes under the
    same names) -> (lines, stderr, return code)"""
    build.build_library()
    c = CASES[case]
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env["MCQ_PROFILE"] = "1"
    if switched:
        env.update(MCQ_INPUT_DEVICE="1", MCQ_INPUT_DEVICE_PIECE=str(PIECE))
    if others:
        env.update(MCQ_FORMAT_DEVICE="1", MCQ_EVALUATE_DEVICE="1")
    if cap_mb is not None:
        env["MCQ_INPUT_DEVICE_MB"] = str(cap_mb)
    with tempfile.TemporaryDirectory() as tmp:
        for f in c["files"]:
            if kind == "golden":
                shutil.copy(os.path.join(GOLD, f), os.path.join(tmp, f))
                continue
            data = inflate_cases.bgzf_file(golden(plain_name(f)), payload=PAYLOAD)
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


def profile(stderr):
    m = RESIDENT.search(stderr)
    assert m, stderr
    return [int(m.group(k)) for k in range(1, 7)], m.group(7)


@pytest.mark.parametrize("kind", ["golden", "bgzf"])
@pytest.mark.parametrize("case", ["everything_species", "pairseq", "two_files", "ground_truth"])
def test_files_are_resident_and_the_lines_are_the_reference_s(case, kind):
    lines, stderr, rc = run(case, kind)
    assert rc == 0, stderr
    assert lines == expected(case)
    (files, pieces, batches, nbytes, records, left), why = profile(stderr)
    names = [plain_name(f) for f in CASES[case]["files"]]
    parsed = [parse_ref.parse(golden(n)) for n in names]
    assert left == 0 and why is None, stderr
    assert files == len(names) and nbytes == sum(len(golden(n)) for n in names) and records == sum(len(p.records) for p in parsed)
    assert all(len(golden(n)) > 2 * PIECE for n in names) and pieces >= 2 * files        # more than one piece per file
    per = 46 if "-pairseq" in CASES[case]["args"] else 23
    assert batches >= sum(-(-len(p.records) // per) for p in parsed)
    assert "inflated on" not in stderr and "parsed on" not in stderr                      # no host inflate, and nobody else's report


@pytest.mark.parametrize("case,kind,resident,reasons", [
    ("fastq_irregular", "golden", 0, ["cli_irregular.fq: irregular at byte "]),
    ("fasta_plus_lines", "golden", 0, ["cli_irregular.fa: irregular at byte "]),
    ("irregular_with_regular", "golden", 1, ["cli_irregular.fa: irregular at byte ", "cli_irregular.fq: irregular at byte "]),
    ("irregular_with_regular", "bgzf", 1, ["cli_irregular.fa: irregular at byte ", "cli_irregular.fq: irregular at byte "]),   # inflated there, copied back once
    ("gzip_input", "golden", 0, ["cli_reads.fa.gz: plain gzip: not BGZF at byte 0"]),
    ("gzip_input", "flipped", 0, ["cli_reads.fa.gz: the device refused block 2 "]),
])
def test_files_the_path_does_not_take_go_the_old_way(case, kind, resident, reasons):
    lines, stderr, rc = run(case, kind)
    assert rc == 0, stderr
    if kind == "flipped":                                                                 # (a file zlib refuses too: what comes out without the switch)
        assert (lines, rc) == run(case, kind, switched=False)[::2]
    else:
        assert lines == expected(case)
    (files, pieces, batches, nbytes, records, left), why = profile(stderr)
    assert files == resident and left == len(reasons) and why is not None, stderr
    named = why.split("; ")
    assert len(named) == len(reasons) and all(n.startswith(r) for n, r in zip(named, reasons)), why
    if resident:                                                                          # the regular file in the middle
        data = golden("cli_pairs.fq")
        assert nbytes == len(data) and records == len(parse_ref.parse(data).records) and pieces >= 2
    for n in named:
        if "irregular at byte" in n:
            f = n.split(":")[0]
            assert n == f"{f}: irregular at byte {parse_ref.parse(golden(f)).offence}", n


def test_pairfiles_stay_on_the_host_and_say_so():
    lines, stderr, rc = run("pairfiles")
    assert rc == 0 and lines == expected("pairfiles")
    assert "mcq: query input read on the host (-pairfiles" in stderr and not RESIDENT.search(stderr)


def test_a_file_larger_than_the_cap_goes_the_old_way():
    lines, stderr, rc = run("everything_species", cap_mb=0)
    assert rc == 0 and lines == expected("everything_species")
    (files, _, _, _, _, left), why = profile(stderr)
    assert files == 0 and left == 1 and why.startswith("cli_reads.fa: larger than the cap of 0 MiB"), stderr


def test_with_the_other_switches():
    for case in ("everything_species", "ground_truth"):
        lines, stderr, rc = run(case, "bgzf", others=True)
        assert rc == 0, stderr
        assert lines == expected(case)
        (files, _, _, _, _, left), _ = profile(stderr)
        assert files == 1 and left == 0, stderr


def test_without_the_switch_nothing_changes():
    for kind in ("golden", "bgzf"):
        lines, stderr, rc = run("two_files", kind, switched=False)
        assert rc == 0 and lines == expected("two_files")
        assert "resident" not in stderr and "query input" not in stderr
