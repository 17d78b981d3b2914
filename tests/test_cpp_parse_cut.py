"""The C++ face of the device cut (include/metacache_amd.hpp): database::parse_cut, driven by examples/parse_cut_example.cpp.  The program
compiles and links without a GPU; on the GPU it must print what the cut rule in plain Python (cut_ref) gives for the same file."""
import os
import subprocess

import pytest

import cut_ref
import parse_cases
import parse_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def example(tmp_path_factory):
    """examples/parse_cut_example.cpp, compiled once into a temporary directory (nothing is written into the source tree)"""
    from metacache_amd import build
    build.build_library()
    exe = str(tmp_path_factory.mktemp("parse_cut_example") / "parse_cut_example")
    cmd = ["g++", "-std=c++14", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "parse_cut_example.cpp"),
           "-L" + os.path.join(ROOT, "metacache_amd", "lib"), "-lmetacache_amd", "-Wl,-rpath," + os.path.join(ROOT, "metacache_amd", "lib"),
           "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def test_parse_cut_example_compiles_and_links(example):
    assert os.path.exists(example)


def run(example, golden, path, R, pairs, open_end):
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return subprocess.run([example, golden.db_path("toy32"), path, str(R), "1" if pairs else "0", "1" if open_end else "0"], env=env, capture_output=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name,R,pairs,open_end", [("cli_reads.fa", 23, False, False), ("cli_pairs.fq", 6, True, False), ("cli_fmt.fa", 1, False, True)])
def test_cpp_output_matches_the_model(golden, example, name, R, pairs, open_end):
    r = run(example, golden, os.path.join(parse_cases.GOLDEN, name), R, pairs, open_end)
    assert r.returncode == 0, r.stderr
    c = cut_ref.cut(parse_cases.golden_bytes(name), R, pairs, open_end)
    assert c.verdict == parse_ref.OK
    want = [b"status\t%d\t%d\t%d\t%d\t%d\t%d" % (c.whole, len(c.cuts) - 1, c.consumed, c.seen, c.longest, c.half)] + [b"%d" % x for x in c.cuts]
    assert r.stdout.split(b"\n")[:-1] == want


@pytest.mark.gpu
def test_cpp_refused_file_says_so(golden, example):
    r = run(example, golden, os.path.join(parse_cases.GOLDEN, "cli_irregular.fq"), 4, False, False)
    c = cut_ref.cut(parse_cases.golden_bytes("cli_irregular.fq"), 4)
    assert c.verdict == parse_ref.IRREGULAR
    assert r.returncode == 3 and r.stdout == b"" and b"verdict 1 at byte %d" % c.offence in r.stderr
