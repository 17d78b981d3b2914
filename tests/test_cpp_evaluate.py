"""The C++ face of the evaluation against a ground truth (include/metacache_amd.hpp): query_host_data::evaluate, database::evaluation and
the classification_statistics mirror, driven by examples/evaluate_example.cpp.  The program compiles and links without a GPU; on the GPU
it must print what the Python binding returns for the same reads and truths."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def example(tmp_path_factory):
    """examples/evaluate_example.cpp, compiled once into a temporary directory (nothing is written into the source tree)"""
    from metacache_amd import build
    build.build_library()
    exe = str(tmp_path_factory.mktemp("evaluate_example") / "evaluate_example")
    cmd = ["g++", "-std=c++14", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "evaluate_example.cpp"),
           "-L" + os.path.join(ROOT, "metacache_amd", "lib"), "-lmetacache_amd", "-Wl,-rpath," + os.path.join(ROOT, "metacache_amd", "lib"),
           "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def test_evaluate_example_compiles_and_links(example):
    assert os.path.exists(example)


@pytest.mark.gpu
@pytest.mark.parametrize("hitmin,coverage", [(0, 0), (5, 1)])
def test_cpp_evaluation_matches_python_binding(golden, example, tmp_path, hitmin, coverage):
    from metacache_amd import api
    single, _, _ = golden.reads()
    reads = [r for r in single[:400] if b"\n" not in r and len(r) > 0]
    db = api.Database.open(golden.db_path("toy32"), max_candidates=2)
    try:
        lin, rank, covered = db.taxon_table()
        rng = np.random.default_rng(9)
        truth = rng.integers(0, len(lin) + 1, len(reads)).astype(np.uint32)           # any taxon, ranked or not, covered or not; 0 = unknown
        f, g = tmp_path / "seqs.txt", tmp_path / "truth.txt"
        f.write_bytes(b"\n".join(reads) + b"\n")
        g.write_text("".join(f"{int(t)}\n" for t in truth))
        env = dict(os.environ)
        env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
        out = subprocess.check_output([example, golden.db_path("toy32"), str(f), str(g), str(hitmin), str(coverage)], env=env).decode().splitlines()
        assigned = db.classify(reads, hitmin=hitmin)
        db.evaluation(reset=True)
        verdicts = db.evaluate(assigned, truth, coverage=bool(coverage))
        ev = db.evaluation()
    finally:
        db.close()
    n = len(reads)
    assert len(out) == n + 21 + 1
    for i, line in enumerate(out[:n]):
        want = (i, int(assigned[i]["taxon"]), int(assigned[i]["rank"]), int(verdicts[i]["known"]), int(verdicts[i]["correct"]), int(verdicts[i]["flags"]) & 1)
        assert line == "\t".join(map(str, want)), (i, line)
    for r, line in enumerate(out[n:n + 21]):
        want = f"rank {r} {ev.assigned(r)} {ev.known(r)} {ev.correct(r)} {ev.wrong(r)} {100 * ev.precision(r):g} {100 * ev.sensitivity(r):g} {ev.coverage(r).false_pos()}"
        assert line == want, (r, line, want)
    assert out[-1] == f"total {ev.total()} unknown {ev.unknown()}"
    assert ev.total() == n and ev.wrong() > 0 and ev.correct() > 0
    assert (sum(ev.coverage(r).false_pos() for r in range(21)) > 0) == bool(coverage)
