"""The C++ face of the all-hits column (include/metacache_amd.hpp): database::set_matches_text, query_host_data::format_matches and the extra
column of query_host_data::format_mappings, driven by examples/matches_example.cpp.  The program compiles and links without a GPU; on
the GPU it must print what the Python binding returns for the same reads, tables and flags."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def example(tmp_path_factory):
    """examples/matches_example.cpp, compiled once into a temporary directory (nothing is written into the source tree)"""
    from metacache_amd import build
    build.build_library()
    exe = str(tmp_path_factory.mktemp("matches_example") / "matches_example")
    cmd = ["g++", "-std=c++14", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "matches_example.cpp"),
           "-L" + os.path.join(ROOT, "metacache_amd", "lib"), "-lmetacache_amd", "-Wl,-rpath," + os.path.join(ROOT, "metacache_amd", "lib"),
           "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def test_matches_example_compiles_and_links(example):
    assert os.path.exists(example)


@pytest.mark.gpu
@pytest.mark.parametrize("windows", [1, 0])
def test_cpp_lines_match_python_binding(golden, example, tmp_path, windows):
    from metacache_amd import api
    single, _, _ = golden.reads()
    reads = [r for r in single[:300] if b"\n" not in r and len(r) > 0]
    db = api.Database.open(golden.db_path("toy32"), max_candidates=2, copy_allhits=1)
    try:
        f = tmp_path / "seqs.txt"
        f.write_bytes(b"\n".join(reads) + b"\n")
        env = dict(os.environ)
        env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
        out = subprocess.check_output([example, golden.db_path("toy32"), str(f), str(windows)], env=env)
        taxa, lin = db.taxa(), db.lineages()
        result = [b"--"] + [f"{t[2]}:{t[3]}".encode() for t in taxa]
        names = [taxa[int(row[0]) - 1][3].encode() if row[0] else b"" for row in lin]
        db.format_set_text(api.TEXT_RESULT, result)
        db.format_set_text(api.TEXT_TARGET_RESULT, [result[int(row[0])] for row in lin])
        db.format_set_text(api.TEXT_CANDIDATE, names)
        db.format_matches_set_text(names)
        cands, _, lists = db.query(reads)
        hits = np.concatenate(lists)
        hit_off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64)
        assigned = db.classify_candidates(cands)
        pieces, piece_off = db.format_matches(hits, hit_off, flags=api.MATCHES_WINDOWS if windows else 0)
        want, off = db.format_mappings(api.format_options(b"\t", db.stride, db.w), cands, assigned, [f"q{i}".encode() for i in range(len(reads))],
                                       flags=api.FORMAT_QUERY_IDS | api.FORMAT_TOPHITS, first_query_id=1, extra=pieces, extra_off=piece_off)
    finally:
        db.close()
    assert out == want
    lines = want.split(b"\n")[:-1]
    assert len(lines) == len(reads) and sum(1 for l in lines if (b"/" in l.split(b"\t")[2]) == bool(windows) and l.split(b"\t")[2].endswith(b",")) > 100
