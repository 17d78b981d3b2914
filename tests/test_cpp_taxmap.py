"""The C++ face of the device ranking pass (include/metacache_amd.hpp): mc_amd::accession_mapper, driven by examples/taxmap_example.cpp.
The program compiles and links without a GPU; on the GPU it must print what the model (taxmap_ref) gives for the same names and tables."""
import os
import subprocess

import pytest

import taxmap_cases as cases
import taxmap_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOY = os.path.join(cases.GOLDEN, "build_in", "taxonomy", "toy.accession2taxid")
NAMES = [(b"55555", 1), (b"AB123456.1", 1), (b"NC_000111.1", 0), (b"NC_000111.1!1", 1), (b"NC_000114.1", 1), (b"NZ_ABCD01000001.1", 1)]


@pytest.fixture(scope="module")
def example(tmp_path_factory):
    """examples/taxmap_example.cpp, compiled once into a temporary directory (nothing is written into the source tree)"""
    from metacache_amd import build
    build.build_library()
    exe = str(tmp_path_factory.mktemp("taxmap_example") / "taxmap_example")
    cmd = ["g++", "-std=c++14", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "taxmap_example.cpp"),
           "-L" + os.path.join(ROOT, "metacache_amd", "lib"), "-lmetacache_amd", "-Wl,-rpath," + os.path.join(ROOT, "metacache_amd", "lib"),
           "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def test_taxmap_example_compiles_and_links(example):
    assert os.path.exists(example)


def run(example, tmp_path, tables):
    names = tmp_path / "names.txt"
    names.write_bytes(b"".join(n + b" %d\n" % w for n, w in reversed(NAMES)))       # (any order: the program sorts them)
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return subprocess.run([example, str(names)] + tables, env=env, capture_output=True)


@pytest.mark.gpu
def test_cpp_output_matches_the_model(example, tmp_path):
    second = tmp_path / "second.accession2taxid"
    second.write_bytes(b"first line\nAB123456\tAB123456.3\t77\t0\nNC_000114\tNC_000114.1\t78\t0\n")
    tables = [TOY, str(tmp_path / "missing.accession2taxid"), str(second)]
    r = run(example, tmp_path, tables)
    assert r.returncode == 0, r.stderr
    m = ref.Model([n for n, _ in NAMES], [w for _, w in NAMES])
    for t in (TOY, str(second)):
        with open(t, "rb") as f:
            data = f.read()
        assert m.add(data[data.index(b"\n") + 1:])[5] == ref.OK
    taxid, key, _ = m.result()
    table_of_call = [0, 2]
    want = [n + (b"\t-" if k == ref.NOT_FOUND else b"\t%d\t%d\t%d" % (t, table_of_call[k >> 32], k & 0xFFFFFFFF)) for (n, _), t, k in zip(NAMES, taxid, key)]
    assert r.stdout.split(b"\n")[:-1] == want
    assert sum(1 for k in key if k != ref.NOT_FOUND) == 4 and key[2] == ref.NOT_FOUND    # (NC_000111.1 has a row and is not wanted)


@pytest.mark.gpu
def test_cpp_refused_table_says_so(example, tmp_path):
    with open(TOY, "rb") as f:
        data = f.read()
    bad = tmp_path / "bad.accession2taxid"
    bad.write_bytes(data.replace(b"\n", b"\r\n"))
    r = run(example, tmp_path, [str(bad)])
    assert r.returncode == 3 and r.stdout == b"" and b"verdict 1 at byte 0" in r.stderr
