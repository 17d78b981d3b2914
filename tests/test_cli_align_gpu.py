"""`mcq query -align` against the output files of the reference's command line (tests/golden/align_expected.json.gz), on databases
`mcq build` made from tests/golden/build_in, run from tests/golden so that the stored source file names resolve.

The reference aligns a read to the record BEFORE its target in the source file (and to nothing where the target opens its file); mcq
aligns to the target's own record.  So the expected file of a case is the reference's recorded file with its alignment lines taken out
and the lines of the plain model (tests/align_ref.py, pinned to the reference by tests/test_align_witness_cpu.py) under mcq's record
rule put in.  The model needs every read's first candidate -- target and window range: they are read off mcq's own -tophits -locations
columns, of the case itself where it prints them, else of a second run with the two options added, whose other columns must be those
of the first run.  Every line outside the alignment lines is the reference's own."""
import gzip
import json
import os
import re
import shutil
import subprocess

import pytest

import align_ref
from metacache_amd import build
from test_cli_gpu import _same

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
NAMES = ["align", "align_tophits", "align_mapped_only", "align_species", "align_maxcand", "align_pairs", "align_long", "align_cov", "align_w64",
         "align_elsewhere"]


def _load(name):
    p = os.path.join(GOLD, name)
    if not os.path.exists(p):
        return {}
    with gzip.open(p, "rt") as f:
        return json.load(f)


EXP = _load("align_expected.json.gz")
CASES = EXP.get("cases", {})
# target name -> (source file, record number) as the reference's own build of these files stored them
SOURCES = {v[2]: (v[3], v[4]) for k, v in _load("build_expected.json.gz").get("build", {}).get("default", {}).get("db", {}).get("taxa", {}).items()
           if int(k) < 0}


@pytest.fixture(scope="module")
def databases(tmp_path_factory):
    if not os.path.exists(build.MCQ):
        build.build_library()
    d = tmp_path_factory.mktemp("align_db")
    for name, extra in EXP["databases"].items():
        r = subprocess.run([build.MCQ, "build", str(d / name)] + EXP["files"] + EXP["tax"] + extra, cwd=GOLD, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
    return d


def _run(databases, c, args, cwd, out, threads=1):
    cmd = [build.MCQ, "query", str(databases / c["db"]), c["reads"]] + args + ["-threads", str(threads), "-no-err", "-out", str(out)]
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    return open(out).read().split("\n")


def _without(line, sep, cols, drop):
    f = line.split(sep)
    return sep.join(x for x, name in zip(f, cols) if name not in drop)


def _run_case(databases, case, tmp_path, threads=1):
    """-> (mcq's lines, the expected lines)"""
    c = CASES[case]
    args = c["args"]
    comment, sep = align_ref.option(args, "-comment", "# "), align_ref.option(args, "-separator", "\t|\t")
    winlen, stride = align_ref.SKETCHING[c["db"]]
    cwd = GOLD
    if c["elsewhere"]:
        cwd = str(tmp_path / "elsewhere")
        os.makedirs(cwd, exist_ok=True)
        shutil.copy(os.path.join(GOLD, c["reads"]), cwd)
    got = _run(databases, c, args, cwd, tmp_path / "out.txt", threads)
    mine = align_ref.parse_output(got, comment)
    if "-tophits" in args and "-locations" in args:
        located = got
    else:                                                   # the same case with the candidates and their ranges shown: its other columns are this run's
        more = [a for a in ("-tophits", "-locations") if a not in args]
        located = _run(databases, c, args + more, cwd, tmp_path / "located.txt", threads)
        lcols = align_ref.columns(located, comment, sep)
        drop = {"top_hits", "candidate_locations"} - set(align_ref.columns(got, comment, sep))
        theirs = align_ref.parse_output(located, comment)
        assert [_without(l, sep, lcols, drop) for _, l, _ in theirs] == [l for _, l, _ in mine], case
        assert [a for _, _, a in theirs] == [a for _, _, a in mine], case
    lcols = align_ref.columns(located, comment, sep)
    top, loc, name_col = lcols.index("top_hits"), lcols.index("candidate_locations"), lcols.index("query_header")
    firsts = [(l.split(sep)[name_col], l.split(sep)[top].split(",")[0], l.split(sep)[loc], l.split(sep)[-1]) for _, l, _ in align_ref.parse_output(located, comment)]
    reads = align_ref.queries(os.path.join(GOLD, c["reads"]), "-pairseq" in args)
    records = align_ref.Records(cwd)
    sequence_level = "-lowest" not in args
    exp, k = [], 0
    ref = c["lines"]
    groups = {i: a for i, _, a in align_ref.parse_output(ref, comment)}
    i = 0
    while i < len(ref):
        exp.append(ref[i])
        if i in groups:
            name, cand, ranges, taxon = firsts[k]
            k += 1
            assert ref[i].split(sep)[align_ref.columns(ref, comment, sep).index("query_header")] == name, (case, i, name)
            if sequence_level and cand and taxon != "--":
                filename, index = SOURCES[cand.rsplit(":", 1)[0]]
                b, e = map(int, re.match(r"^\[(\d+),(\d+)\]", ranges).groups())
                read, mate = reads[name]
                if "-cov-percentile" in args:               # the reference keeps no sequences for the pass after the coverage filter: an empty query
                    read, mate = b"", None
                lines = align_ref.alignment_lines(records, "mcq", comment, filename, index, b // stride, (e - winlen) // stride, winlen, stride, read, mate)
                if lines:
                    exp += lines
            if groups[i] is not None:
                i += 3
        i += 1
    assert k == len(firsts), (case, k, len(firsts))
    return got, exp


@pytest.mark.gpu
@pytest.mark.parametrize("case", NAMES)
def test_cli_align_matches_reference_lines_and_model_alignments(case, databases, tmp_path):
    got, exp = _run_case(databases, case, tmp_path)
    n = sum("  score  " in l for l in exp)
    assert (n == 0) == (case in ("align_species", "align_elsewhere")), (case, n)
    _same(got, exp, case)


@pytest.mark.gpu
def test_targets_that_open_their_file_are_aligned(databases, tmp_path):
    """the case the reference drops: per source file, a read whose first candidate is the file's first record gets its alignment"""
    c = CASES["align_tophits"]
    got = _run(databases, c, c["args"], GOLD, tmp_path / "out.txt")
    sep = "\t|\t"
    top = align_ref.columns(got, "# ", sep).index("top_hits")
    seen = {}
    for _, line, aln in align_ref.parse_output(got, "# "):
        cand = line.split(sep)[top].split(",")[0]
        if cand and line.split(sep)[-1] != "--":
            filename, index = SOURCES[cand.rsplit(":", 1)[0]]
            if index == 0:
                assert aln is not None and aln[0].startswith(f"#   score  ") and f"aligned to {filename} #0 in range" in aln[0], line[:120]
                seen[filename] = seen.get(filename, 0) + 1
    assert len(seen) == 4, seen


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["align_tophits", "align_pairs", "align_long"])
def test_threads_do_not_change_the_output(case, databases, tmp_path):
    c = CASES[case]
    one = _run(databases, c, c["args"] + ["-batch-size", "16"], GOLD, tmp_path / "one.txt", 1)
    eight = _run(databases, c, c["args"] + ["-batch-size", "16"], GOLD, tmp_path / "eight.txt", 8)
    _same(eight, one, case)
    assert sum("  score  " in l for l in one) > 5
