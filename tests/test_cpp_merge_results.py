"""The C++ face of the device merge (include/metacache_amd.hpp): mc_amd::result_merger, driven by examples/merge_results_example.cpp.  The
program compiles and links without a GPU; on the GPU it must print what the witness (merge_results_ref) gives for the same files."""
import os
import subprocess

import pytest

import merge_results_cases as cases
import merge_results_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def example(tmp_path_factory):
    """examples/merge_results_example.cpp, compiled once into a temporary directory (nothing is written into the source tree)"""
    from metacache_amd import build
    build.build_library()
    exe = str(tmp_path_factory.mktemp("merge_results_example") / "merge_results_example")
    cmd = ["g++", "-std=c++14", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "merge_results_example.cpp"),
           "-L" + os.path.join(ROOT, "metacache_amd", "lib"), "-lmetacache_amd", "-Wl,-rpath," + os.path.join(ROOT, "metacache_amd", "lib"),
           "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def test_merge_results_example_compiles_and_links(example):
    assert os.path.exists(example)


def run(example, tmp_path, max_cand, paths):
    ids, lin, rank, _ = cases.toy_table()
    taxa = tmp_path / "taxa.txt"
    taxa.write_text("".join(f"{int(i)} {int(r)} {' '.join(str(int(x)) for x in row)}\n" for i, r, row in zip(ids, rank, lin)))
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return subprocess.run([example, str(taxa), str(max_cand)] + paths, env=env, capture_output=True)


@pytest.mark.gpu
@pytest.mark.parametrize("names,max_cand", [(("merge_in/part0.txt", "merge_in/part1.txt"), 4), (("merge_cases_in/c.txt", "merge_cases_in/a.txt", "merge_cases_in/b.txt"), 8)])
def test_cpp_output_matches_the_witness(example, tmp_path, names, max_cand):
    ids, lin, rank, _ = cases.toy_table()
    r = run(example, tmp_path, max_cand, [os.path.join(cases.GOLDEN, n) for n in names])
    assert r.returncode == 0, r.stderr
    m = ref.Merger(ids, lin, rank, 1024, max_cand, 4)
    datas = []
    for n in names:
        with open(os.path.join(cases.GOLDEN, n), "rb") as f:
            datas.append(f.read())
        assert m.add(datas[-1], cases.tophits_column(datas[-1]))[5] == ref.OK
    out = m.classify(5, 1.0, 19)
    want = []
    for q in range(m.count):
        call, off, length = m.hdr[q]
        hits = ",".join(f"{int(ids[x - 1])}:{h}" for x, h in m.lists[q])
        taxon, rk, _ = map(int, out[q])
        want.append(f"{q + 1}\t{datas[call][off:off + length].decode()}\t{hits}\t{int(ids[taxon - 1]) if taxon else 0}\t{rk}".encode())
    assert r.stdout.split(b"\n")[:-1] == want


@pytest.mark.gpu
def test_cpp_refused_file_says_so(example, tmp_path):
    ids, _, rank, _ = cases.toy_table()
    data, at = cases.irregular_files(ids, rank)["crlf"]
    bad = tmp_path / "bad.txt"
    bad.write_bytes(data)
    r = run(example, tmp_path, 2, [os.path.join(cases.GOLDEN, "merge_cases_in/a.txt"), str(bad)])
    assert r.returncode == 3 and r.stdout == b"" and b"verdict 1 at byte %d" % at in r.stderr
