"""The C++ face of the mapping lines (include/metacache_amd.hpp): database::set_mapping_text and query_host_data::format_mappings, driven
by examples/format_example.cpp.  The program compiles and links without a GPU; on the GPU it must print what the Python binding returns
for the same reads, tables and flags."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def example(tmp_path_factory):
    """examples/format_example.cpp, compiled once into a temporary directory (nothing is written into the source tree)"""
    from metacache_amd import build
    build.build_library()
    exe = str(tmp_path_factory.mktemp("format_example") / "format_example")
    cmd = ["g++", "-std=c++14", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "format_example.cpp"),
           "-L" + os.path.join(ROOT, "metacache_amd", "lib"), "-lmetacache_amd", "-Wl,-rpath," + os.path.join(ROOT, "metacache_amd", "lib"),
           "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def test_format_example_compiles_and_links(example):
    assert os.path.exists(example)


@pytest.mark.gpu
@pytest.mark.parametrize("hitmin,flags", [(0, 2 | 8), (5, 2 | 8 | 16 | 32)])
def test_cpp_lines_match_python_binding(golden, example, tmp_path, hitmin, flags):
    from metacache_amd import api
    single, _, _ = golden.reads()
    reads = [r for r in single[:400] if b"\n" not in r and len(r) > 0]
    db = api.Database.open(golden.db_path("toy32"), max_candidates=2)
    try:
        f = tmp_path / "seqs.txt"
        f.write_bytes(b"\n".join(reads) + b"\n")
        env = dict(os.environ)
        env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
        out = subprocess.check_output([example, golden.db_path("toy32"), str(f), str(hitmin), str(flags)], env=env)
        taxa, lin = db.taxa(), db.lineages()
        result = [b"--"] + [f"{t[2]}:{t[3]}".encode() for t in taxa]
        db.format_set_text(api.TEXT_RESULT, result)
        db.format_set_text(api.TEXT_TARGET_RESULT, [result[int(row[0])] for row in lin])
        db.format_set_text(api.TEXT_CANDIDATE, [taxa[int(row[0]) - 1][3].encode() if row[0] else b"" for row in lin])
        cands, _, _ = db.query(reads)
        assigned = db.classify_candidates(cands, hitmin=hitmin)
        want, off = db.format_mappings(api.format_options(b"\t", db.stride, db.w), cands, assigned, [f"q{i}".encode() for i in range(len(reads))],
                                       flags=flags, first_query_id=1)
    finally:
        db.close()
    assert out == want
    lines = want.split(b"\n")[:-1]
    assert (len(lines) < len(reads)) == bool(flags & 32) and len(lines) > 100 and all(l.split(b"\t")[1].startswith(b"q") for l in lines)
