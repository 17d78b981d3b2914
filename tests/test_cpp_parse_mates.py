"""The C++ face of the mates parse (include/metacache_amd.hpp): database::parse_mates and query_batch::add_file_mates, driven by
examples/parse_mates_example.cpp.  The program compiles and links without a GPU; on the GPU it must print what the mates rule in plain
Python (parse_mates_ref) gives for the same two files, and the candidates the Python binding returns for their pairs."""
import os
import subprocess

import pytest

import parse_cases
import parse_mates_ref as mref
import parse_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def example(tmp_path_factory):
    """examples/parse_mates_example.cpp, compiled once into a temporary directory (nothing is written into the source tree)"""
    from metacache_amd import build
    build.build_library()
    exe = str(tmp_path_factory.mktemp("parse_mates_example") / "parse_mates_example")
    cmd = ["g++", "-std=c++14", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "parse_mates_example.cpp"),
           "-L" + os.path.join(ROOT, "metacache_amd", "lib"), "-lmetacache_amd", "-Wl,-rpath," + os.path.join(ROOT, "metacache_amd", "lib"),
           "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def test_parse_mates_example_compiles_and_links(example):
    assert os.path.exists(example)


def run(example, golden, path1, path2):
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return subprocess.run([example, golden.db_path("toy32"), path1, path2], env=env, capture_output=True)


@pytest.mark.gpu
def test_cpp_output_matches_the_model(golden, example):
    from metacache_amd import api
    p1, p2 = (os.path.join(parse_cases.GOLDEN, n) for n in ("cli_p1.fa", "cli_p2.fa"))
    r = run(example, golden, p1, p2)
    assert r.returncode == 0, r.stderr
    d1, d2 = parse_cases.golden_bytes("cli_p1.fa"), parse_cases.golden_bytes("cli_p2.fa")
    m = mref.mates(d1, d2)
    want = [b"%s\t%d\t%d\t%s\t%s" % (m["names"][int(m["name_off"][q]):int(m["name_off"][q + 1])], m["qinfo"][q, 1], m["qinfo"][q, 3],
                                    d1[int(m["hdr"][2 * q, 0]):int(m["hdr"][2 * q, 0]) + int(m["hdr"][2 * q, 1])],
                                    d2[int(m["hdr"][2 * q + 1, 0]):int(m["hdr"][2 * q + 1, 0]) + int(m["hdr"][2 * q + 1, 1])]) for q in range(len(m["qinfo"]))]
    reads, mates = [x[2] for x in parse_ref.parse(d1).records], [x[2] for x in parse_ref.parse(d2).records]
    db = api.Database.open(golden.db_path("toy32"), max_candidates=2)
    try:
        cands, _, _ = db.query(reads, mates)
    finally:
        db.close()
    want += [b"%d\t%d" % (c[0]["tgt"], c[0]["hits"]) if c[0]["hits"] else b"-\t0" for c in cands]
    assert r.stdout.split(b"\n")[:-1] == want


@pytest.mark.gpu
def test_cpp_unequal_files_say_so(golden, example, tmp_path):
    d2 = parse_cases.golden_bytes("cli_p2.fa") + b">one more\nACGT\n"
    longer = tmp_path / "longer.fa"
    longer.write_bytes(d2)
    n = len(parse_ref.parse(d2).records)
    r = run(example, golden, os.path.join(parse_cases.GOLDEN, "cli_p1.fa"), str(longer))
    assert r.returncode == 3 and r.stdout == b"" and b"%d records beside %d" % (n - 1, n) in r.stderr
