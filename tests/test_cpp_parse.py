"""The C++ face of the device parse (include/metacache_amd.hpp): database::parse_records, query_batch::add_file_bytes and
query_host_data::records, driven by examples/parse_example.cpp.  The program compiles and links without a GPU; on the GPU it must print
what the record rule in plain Python (parse_ref) gives for the same file, and the candidates the Python binding returns for its reads."""
import os
import subprocess

import pytest

import parse_cases
import parse_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def example(tmp_path_factory):
    """examples/parse_example.cpp, compiled once into a temporary directory (nothing is written into the source tree)"""
    from metacache_amd import build
    build.build_library()
    exe = str(tmp_path_factory.mktemp("parse_example") / "parse_example")
    cmd = ["g++", "-std=c++14", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "parse_example.cpp"),
           "-L" + os.path.join(ROOT, "metacache_amd", "lib"), "-lmetacache_amd", "-Wl,-rpath," + os.path.join(ROOT, "metacache_amd", "lib"),
           "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def test_parse_example_compiles_and_links(example):
    assert os.path.exists(example)


def run(example, golden, path, pairs):
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return subprocess.run([example, golden.db_path("toy32"), path, "1" if pairs else "0"], env=env, capture_output=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name,pairs", [("cli_reads.fa", False), ("cli_pairs.fq", True), ("cli_fmt.fa", True)])
def test_cpp_output_matches_the_model(golden, example, name, pairs):
    from metacache_amd import api
    path = os.path.join(parse_cases.GOLDEN, name)
    r = run(example, golden, path, pairs)
    assert r.returncode == 0, r.stderr
    data = parse_cases.golden_bytes(name)
    parsed = parse_ref.parse(data)
    reads, mates = parse_ref.reads_of(parsed, pairs)
    heads = parsed.records[0::2] if pairs else parsed.records
    want = [b"%s\t%d\t%d\t%s" % (parse_ref.name_of(data, h[0], h[1]), len(reads[q]), len(mates[q]) if pairs else 0, data[h[0]:h[0] + h[1]])
            for q, h in enumerate(heads)]
    db = api.Database.open(golden.db_path("toy32"), max_candidates=2)
    try:
        cands, _, _ = db.query(reads, mates)
    finally:
        db.close()
    want += [b"%d\t%d" % (c[0]["tgt"], c[0]["hits"]) if c[0]["hits"] else b"-\t0" for c in cands]
    assert r.stdout.split(b"\n")[:-1] == want


@pytest.mark.gpu
def test_cpp_refused_file_says_so(golden, example):
    r = run(example, golden, os.path.join(parse_cases.GOLDEN, "cli_irregular.fa"), False)
    data = parse_cases.golden_bytes("cli_irregular.fa")
    assert r.returncode == 3 and r.stdout == b"" and b"verdict 1 at byte %d" % parse_ref.parse(data).offence in r.stderr
