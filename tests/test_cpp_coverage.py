"""The -cov-percentile faces that no other test calls.

C++ mirror (include/metacache_amd.hpp): query_host_data::cover, database::keep_by_coverage and query_host_data::classify_kept, driven by
examples/coverage_example.cpp; on the GPU the program must print what Database.classify_by_coverage returns for the same reads.
mcq: a -cov-percentile run takes its covered-window counts from the library (it says so under MCQ_PROFILE) and never falls back to the
host loop without a note on stderr."""
import gzip
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def example(tmp_path_factory):
    """examples/coverage_example.cpp, compiled once into a temporary directory (nothing is written into the source tree)"""
    from metacache_amd import build
    build.build_library()
    exe = str(tmp_path_factory.mktemp("coverage_example") / "coverage_example")
    cmd = ["g++", "-std=c++14", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "coverage_example.cpp"),
           "-L" + os.path.join(ROOT, "metacache_amd", "lib"), "-lmetacache_amd", "-Wl,-rpath," + os.path.join(ROOT, "metacache_amd", "lib"),
           "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def test_coverage_example_compiles_and_links(example):
    assert os.path.exists(example)


@pytest.mark.gpu
@pytest.mark.parametrize("percentile,hitmin", [(0.0, 0), (0.3, 2)])
def test_cpp_two_passes_match_python_binding(golden, example, tmp_path, percentile, hitmin):
    from metacache_amd import api
    exe = example
    single, _, _ = golden.reads()
    reads = [r for r in single[:400] if b"\n" not in r and len(r) > 0]
    f = tmp_path / "seqs.txt"
    f.write_bytes(b"\n".join(reads) + b"\n")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    out = subprocess.check_output([exe, golden.db_path("toy32"), str(f), str(percentile), str(hitmin)], env=env).decode().splitlines()
    db = api.Database.open(golden.db_path("toy32"), max_candidates=2)
    try:
        cands, _, _ = db.query(reads)
        db.coverage_counts(reset=True)
        db.coverage_add(cands, hitmin=hitmin)
        covered, windows, _ = db.coverage_counts(reset=True)
        keep = api.coverage_keep(covered, windows, percentile)
        want = db.classify_by_coverage(reads, percentile=percentile, hitmin=hitmin)
    finally:
        db.close()
    assert (covered > 0).sum() >= 2
    if percentile > 0:
        assert 0 < keep.sum() < (covered > 0).sum()          # (the case drops something, and not everything)
    assert out[0] == f"kept {int(keep.sum())}"
    assert len(out) == 1 + len(reads)
    for i, line in enumerate(out[1:]):
        assert line == f"{i}\t{int(want[i]['taxon'])}\t{int(want[i]['rank'])}", (i, line)
    assert any(int(w["taxon"]) for w in want)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["cov_percentile", "cov_percentile_species"])
def test_mcq_counts_covered_windows_on_the_device(case, tmp_path):
    from metacache_amd import build
    build.build_library()
    with gzip.open(os.path.join(GOLD, "cli_expected.json.gz"), "rt") as fh:
        c = json.load(fh)[case]
    env = dict(os.environ)
    env["MCQ_PROFILE"] = "1"
    cmd = [build.MCQ, "query", "toy32"] + c["files"] + c["args"] + ["-threads", "1", "-out", str(tmp_path / "out.txt")]
    r = subprocess.run(cmd, cwd=GOLD, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr
    assert "counted on the host" not in r.stderr, r.stderr
    m = re.search(r"coverage on the device: (\d+) mc_coverage_add calls, (\d+) candidates marked, (\d+) windows covered", r.stderr)
    assert m, r.stderr
    assert int(m.group(1)) > 0 and int(m.group(2)) > 0 and int(m.group(3)) > 0
