"""The C++ face of the device inflate (include/metacache_amd.hpp): mc_amd::bgzf_index and database::inflate, driven by
examples/inflate_example.cpp.  The program compiles and links without a GPU; on the GPU its stdout must be what gzip gives for a BGZF
file, and a file that is not BGZF or that the device refuses must end with exit code 3 and the verdict on stderr."""
import gzip
import os
import subprocess

import pytest

import inflate_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def example(tmp_path_factory):
    """examples/inflate_example.cpp, compiled once into a temporary directory (nothing is written into the source tree)"""
    from metacache_amd import build
    build.build_library()
    exe = str(tmp_path_factory.mktemp("inflate_example") / "inflate_example")
    cmd = ["g++", "-std=c++14", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "inflate_example.cpp"),
           "-L" + os.path.join(ROOT, "metacache_amd", "lib"), "-lmetacache_amd", "-Wl,-rpath," + os.path.join(ROOT, "metacache_amd", "lib"),
           "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def test_inflate_example_compiles_and_links(example):
    assert os.path.exists(example)


def test_library_does_not_link_zlib():
    from metacache_amd import build
    build.build_library()
    r = subprocess.run(["readelf", "-d", build.LIB], capture_output=True, text=True)
    assert r.returncode == 0 and "NEEDED" in r.stdout and "libz" not in r.stdout


def run(example, golden, path):
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return subprocess.run([example, golden.db_path("toy32"), path], env=env, capture_output=True)


@pytest.mark.gpu
def test_cpp_output_equals_gzip(golden, example, tmp_path):
    with open(os.path.join(GOLDEN, "cli_pairs.fq"), "rb") as f:
        data = inflate_cases.bgzf_file(f.read(), payload=5000)
    path = tmp_path / "pairs.fq.gz"
    path.write_bytes(data)
    r = run(example, golden, str(path))
    assert r.returncode == 0, r.stderr
    assert r.stdout == gzip.decompress(data) and b"ok: " in r.stderr


@pytest.mark.gpu
def test_cpp_foreign_and_corrupt_files_say_so(golden, example, tmp_path):
    r = run(example, golden, os.path.join(GOLDEN, "cli_reads.fa.gz"))
    assert r.returncode == 3 and r.stdout == b"" and b"foreign at byte 0" in r.stderr
    good = inflate_cases.good_cases()
    data = good["short_text"][0] + inflate_cases.bad_cases()["wrong_crc"] + good["one_byte"][0] + inflate_cases.EOF_BLOCK
    path = tmp_path / "bad.gz"
    path.write_bytes(data)
    r = run(example, golden, str(path))
    assert r.returncode == 3 and r.stdout == b"" and b"corrupt block 1 reason 10" in r.stderr
