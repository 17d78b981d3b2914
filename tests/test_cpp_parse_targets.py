"""The C++ face of the target parse (include/metacache_amd.hpp): mc_amd::parsed_targets and database::parse_targets, driven by
examples/parse_targets_example.cpp.  The program compiles and links without a GPU; on the GPU it must print what the target rule in plain
Python (targets_ref) gives for the same files, and the database it writes must hold exactly those targets."""
import os
import subprocess

import pytest

import targets_cases
import targets_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def example(tmp_path_factory):
    """examples/parse_targets_example.cpp, compiled once into a temporary directory (nothing is written into the source tree)"""
    from metacache_amd import build
    build.build_library()
    exe = str(tmp_path_factory.mktemp("parse_targets_example") / "parse_targets_example")
    cmd = ["g++", "-std=c++14", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "parse_targets_example.cpp"),
           "-L" + os.path.join(ROOT, "metacache_amd", "lib"), "-lmetacache_amd", "-Wl,-rpath," + os.path.join(ROOT, "metacache_amd", "lib"),
           "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def test_parse_targets_example_compiles_and_links(example):
    assert os.path.exists(example)


def fnv(seq):
    h = 14695981039346656037
    for c in seq:
        h = ((h ^ c) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def run(example, db, paths):
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return subprocess.run([example, db] + paths, env=env, capture_output=True, timeout=300)


@pytest.mark.gpu
def test_cpp_output_matches_the_model(example, tmp_path):
    from test_cli_build_gpu import parse_db
    paths = [os.path.join(targets_cases.GENOMES, n) for n in targets_cases.GENOME_FILES]
    extra = tmp_path / "empty_records.fa"
    extra.write_bytes(b">e0 an empty one first\n>e1 x\nACGTTGCAACGTTGCAACGTAGCATCGATCGATTAGCAGCATCGACTAGCATCGACTACGACTAGCATCAGCATCAGCATTTTAGAGAGCGCGCATATCGAGCGACTACGATCAGCGGACTATATTCGAG\n>e2 last, no newline")
    paths.append(str(extra))
    files = [open(p, "rb").read() for p in paths]
    parsed = targets_ref.parse(files)
    assert parsed.verdict == targets_ref.OK
    data = b"".join(files)
    db = str(tmp_path / "written")
    r = run(example, db, paths)
    assert r.returncode == 0, r.stderr
    with_seq = [rec for rec in parsed.records if rec[2]]
    want = [b"status\t%d\t%d\t%d" % (len(parsed.records), len(with_seq), max(len(rec[2]) for rec in parsed.records))]
    want += [b"%d\t%d\t%s\t%d\t%x" % (f, i, data[h:h + hl], len(s), fnv(s)) for h, hl, s, f, i in parsed.records]
    want.append(b"written\t%s\t%d targets" % (db.encode(), len(with_seq)))
    assert r.stdout.split(b"\n")[:-1] == want
    got = parse_db(db)
    assert got["targets"] == len(with_seq)
    for t, (h, hl, s, f, i) in enumerate(with_seq):
        parent, rank, name, filename, index, windows = got["taxa"][str(-t - 1)]
        assert (name, filename, index) == (data[h:h + hl].split(b" ")[0].decode(), paths[f], i), t


@pytest.mark.gpu
def test_cpp_refused_range_says_so(example, tmp_path):
    good = os.path.join(targets_cases.GENOMES, targets_cases.GENOME_FILES[0])
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"@r\nACGT\n+\nIIII\n")
    r = run(example, str(tmp_path / "never"), [good, str(fq)])
    assert r.returncode == 3 and r.stdout == b"" and b"verdict 1 at byte %d in file 1" % os.path.getsize(good) in r.stderr
    assert not os.path.exists(str(tmp_path / "never.meta"))
