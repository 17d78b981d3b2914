"""The C++ face of the device inflate of whole gzip files (include/metacache_amd.hpp): mc_amd::gzip_hint and database::inflate_streams,
driven by examples/inflate_streams_example.cpp.  The program compiles and links without a GPU; on the GPU its stdout must be what zlib
gives for the files it takes, and every file that the hint or the device leaves out must be named on stderr with its reason, with exit
code 3."""
import gzip
import os
import subprocess

import pytest

import gzip_cases
import gzip_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def example(tmp_path_factory):
    """examples/inflate_streams_example.cpp, compiled once into a temporary directory (nothing is written into the source tree)"""
    from metacache_amd import build
    build.build_library()
    exe = str(tmp_path_factory.mktemp("inflate_streams_example") / "inflate_streams_example")
    cmd = ["g++", "-std=c++14", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "inflate_streams_example.cpp"),
           "-L" + os.path.join(ROOT, "metacache_amd", "lib"), "-lmetacache_amd", "-Wl,-rpath," + os.path.join(ROOT, "metacache_amd", "lib"),
           "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def test_inflate_streams_example_compiles_and_links(example):
    assert os.path.exists(example)


def run(example, golden, paths):
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return subprocess.run([example, golden.db_path("toy32")] + [str(p) for p in paths], env=env, capture_output=True)


@pytest.mark.gpu
def test_cpp_output_equals_zlib(golden, example, tmp_path):
    good = gzip_cases.good_cases()
    names = ["fname", "one_member_200000", "fextra_fname_fcomment", "empty_file"]
    paths = []
    for n in names:
        paths.append(tmp_path / (n + ".fa.gz"))
        paths[-1].write_bytes(good[n][0])
    paths.append(os.path.join(GOLDEN, "build_in", "genomes", "more.fa.gz"))
    with open(paths[-1], "rb") as f:
        more = gzip.decompress(f.read())
    r = run(example, golden, paths)
    assert r.returncode == 0, r.stderr
    assert r.stdout == b"".join(good[n][1] for n in names) + more
    assert r.stderr.count(b": ok 1 members ") == 5 and b"one_member_200000.fa.gz: ok 1 members 200000 bytes" in r.stderr


@pytest.mark.gpu
def test_cpp_files_left_out_say_so(golden, example, tmp_path):
    good, bad = gzip_cases.good_cases(), gzip_cases.bad_cases()
    text = good["ftext"][1]
    files = {"a.gz": good["fname"][0], "fhcrc.gz": bad["fhcrc"][0], "chain.gz": good["chain_of_3"][0], "crc.gz": gzip_cases.member(gzip_cases.raw_deflate(text), text, crc=1),
             "b.gz": good["ftext"][0], "tail.gz": bad["trailing_zeros"][0]}
    paths = []
    for n, data in files.items():
        paths.append(tmp_path / n)
        paths[-1].write_bytes(data)
    r = run(example, golden, paths)
    assert r.returncode == 3, r.stderr
    assert r.stdout == good["fname"][1] + good["ftext"][1]                          # the good files' bytes, whatever their neighbours are
    assert b"fhcrc.gz: foreign reason %d\n" % gzip_ref.R_HEADER in r.stderr
    assert b"chain.gz: refused reason %d\n" % gzip_ref.R_OVER in r.stderr          # the trailing ISIZE of a chain is too small: stated
    assert b"crc.gz: refused reason %d\n" % gzip_ref.R_CRC in r.stderr
    # (trailing zeros: the last four bytes are the room, 0, and the first member does not fit it)
    assert b"tail.gz: refused reason %d\n" % gzip_ref.R_OVER in r.stderr
    assert b"a.gz: ok 1 members 3000 bytes" in r.stderr and b"b.gz: ok 1 members 3000 bytes" in r.stderr
