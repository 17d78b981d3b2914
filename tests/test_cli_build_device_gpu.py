"""`mcq build` / `modify` / `build+query` with MCQ_BUILD_PARSE_DEVICE=1 (TargetParseStep, mcq_build.h): the plain FASTA files of every case
of tests/golden/build_expected.json.gz go through mc_parse_targets, and the databases and query lines are those of the goldens -- which
the reference's own `build` made.  The profile line must report every plain '>' file of the case on the device and name the others with
their reasons.  With MCQ_BUILD_PARSE_PIECE=4096 every file is cut into ranges, pieces double where a record is longer, and the record
numbers continue across a file's ranges: the same databases.  A FASTQ file among the genomes goes to the host loop: the run equals the
run with the switch unset.  (The switch unset is test_cli_build_gpu.py's ground.)"""
import os
import re
import shutil
import subprocess

import pytest

from metacache_amd import build
from test_cli_build_gpu import EXP, GOLD, parse_db, same_db
from test_cli_gpu import _same

pytestmark = pytest.mark.gpu
PLAIN = {"GCF_000001111.1_ASM111v1_genomic.fna", "mixed.fa", "GCF_000002222.2_other.fa"}
LINE = re.compile(r"^mcq profile: reference sequences parsed on the device: (\d+) mc_parse_targets calls, (\d+) bytes, (\d+) records, (\d+) targets, "
                  r"kernels (\S+) \+ (\S+) ms, (\d+) files, (\d+) files left to the host(?: \((.*)\))?$", re.M)


def run(mode, args, env_extra, **kw):
    env = dict(os.environ, MCQ_BUILD_PARSE_DEVICE="1", MCQ_PROFILE="1")
    env.update(env_extra)
    for k in [k for k, v in env.items() if v is None]:
        del env[k]
    r = subprocess.run([build.MCQ, mode] + args, cwd=GOLD, capture_output=True, text=True, timeout=600, env=env, **kw)
    assert r.returncode == 0, (mode, r.stderr)
    return r


def inputs_of(args):
    """the sequence files a case names (directories expanded), by base name"""
    names = []
    for a in args:
        if a.startswith("-"):
            break
        p = os.path.join(GOLD, a)
        names += sorted(os.listdir(p)) if os.path.isdir(p) else [os.path.basename(a)]
    return names


def check_profile(stderr, files, tag, cut=False):
    m = LINE.search(stderr)
    assert m, (tag, stderr[-2000:])
    calls, nbytes, records, targets, _, _, on_device, left, listed = m.groups()
    plain = [f for f in files if f in PLAIN]
    assert int(on_device) == len(plain) and int(left) == len(files) - len(plain), (tag, m.group(0))
    assert int(nbytes) == sum(os.path.getsize(os.path.join(GOLD, "build_in", "genomes", "sub" if f.startswith("GCF_000002222") else "", f)) for f in plain), (tag, m.group(0))
    if plain:
        assert int(records) >= int(targets) > 0 and int(calls) >= (2 * len(plain) if cut else 1), (tag, m.group(0))
    else:
        assert (int(calls), int(records), int(targets)) == (0, 0, 0), (tag, m.group(0))
    reasons = dict(x.rsplit(": ", 1) for x in listed.split("; ")) if listed else {}
    assert sorted(os.path.basename(x.rsplit(": ", 1)[0]) for x in (listed.split("; ") if listed else [])) == sorted(f for f in files if f not in PLAIN), (tag, listed)
    for k, why in reasons.items():
        if k.endswith("more.fa.gz"):
            assert why == "gzip", (tag, listed)
        if k.endswith("assembly_summary.txt"):
            assert why == "does not begin with '>'", (tag, listed)
    if reasons:
        assert "parsed on the host" in stderr, tag


def query(db, tmp_path, want, tag):
    out = tmp_path / "q.txt"
    r = subprocess.run([build.MCQ, "query", db, "build_reads.fa"] + EXP["query_args"] + ["-threads", "1", "-out", str(out)], cwd=GOLD, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    _same(out.read_text().split("\n"), want, tag)


@pytest.mark.parametrize("case", sorted(EXP["build"]))
def test_build_on_the_device_writes_the_reference_database(case, tmp_path):
    c = EXP["build"][case]
    db = str(tmp_path / case)
    r = run("build", [db] + c["args"] + c["mcq_extra"], {})
    check_profile(r.stderr, inputs_of(c["args"]), case)
    same_db(parse_db(db), c["db"], case)
    query(db, tmp_path, c["query"], case)


@pytest.mark.parametrize("case", sorted(EXP.get("modify", {})))
def test_modify_on_the_device_adds_to_a_database(case, tmp_path):
    c = EXP["modify"][case]
    db = str(tmp_path / case)
    for mode, args in (("build", c["first"] + c["mcq_extra"]), ("modify", c["second"])):
        r = run(mode, [db] + args, {})
        check_profile(r.stderr, inputs_of(args) * (2 if mode == "modify" else 1), (case, mode))   # (modify adds every new file twice, as the reference does)
    same_db(parse_db(db), c["db"], case)
    query(db, tmp_path, c["query"], case)


@pytest.mark.parametrize("case", sorted(EXP["bq"]))
def test_build_query_on_the_device(case, tmp_path):
    c = EXP["bq"][case]
    out, saved = tmp_path / "bq.txt", str(tmp_path / "saved")
    r = run("build+query", [a.format(savedb=saved) for a in c["args"]] + ["-threads", "1", "-out", str(out)], {})
    check_profile(r.stderr, ["mixed.fa"], case)
    _same(out.read_text().split("\n"), c["lines"], case)
    if "saved" in c:
        same_db(parse_db(saved), c["saved"], case)


@pytest.mark.parametrize("kind,case", [(kind, case) for kind in ("build", "modify", "bq") for case in sorted(EXP.get(kind, {}))])
def test_small_pieces_cut_the_files_and_give_the_same_database(kind, case, tmp_path):
    """(same_db compares every target's record number inside its file: the numbers continued across the file's ranges)"""
    env = {"MCQ_BUILD_PARSE_PIECE": "4096"}
    c = EXP[kind][case]
    db = str(tmp_path / case)
    if kind == "build":
        r = run("build", [db] + c["args"] + c["mcq_extra"], env)
        check_profile(r.stderr, inputs_of(c["args"]), case, cut=True)
        same_db(parse_db(db), c["db"], case)
    elif kind == "modify":
        for mode, args in (("build", c["first"] + c["mcq_extra"]), ("modify", c["second"])):
            r = run(mode, [db] + args, env)
            check_profile(r.stderr, inputs_of(args) * (2 if mode == "modify" else 1), (case, mode), cut=True)
        same_db(parse_db(db), c["db"], case)
    else:
        out = tmp_path / "bq.txt"
        r = run("build+query", [a.format(savedb=db) for a in c["args"]] + ["-threads", "1", "-out", str(out)], env)
        check_profile(r.stderr, ["mixed.fa"], case, cut=True)
        _same(out.read_text().split("\n"), c["lines"], case)
        if "saved" in c:
            same_db(parse_db(db), c["saved"], case)


def ranges_of(data, cap):
    """the driver's cut of a file larger than a piece: at the last "\\n>" inside the room, the room doubling where there is none"""
    out, pos = [], 0
    while pos < len(data):
        n = min(len(data) - pos, cap)
        if pos + n < len(data):
            q = data.rfind(b"\n>", pos, pos + n)
            if q < 0:
                cap *= 2
                continue
            n = q + 1 - pos
        out.append((pos, pos + n))
        pos += n
    return out


def test_a_record_longer_than_the_piece_doubles_it(tmp_path):
    """records of 20 000 bases between small ones and an empty one, pieces of 4 096 bytes: the same database as with one piece and as on
    the host, the record numbers continuing across the file's ranges"""
    import numpy as np
    rng = np.random.default_rng(3)
    dna = lambda n: np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()
    wrap = lambda s: b"\n".join(s[k:k + 60] for k in range(0, len(s), 60)) + b"\n"
    data = (b">s1 first\n" + wrap(dna(900)) + b">s2 a long one\n" + wrap(dna(20000)) + b">s3\n>s4 after an empty one\n" + wrap(dna(700)) +
            b">s5 long again\n" + wrap(dna(20000)) + b">s6\n" + wrap(dna(900)))
    ranges = ranges_of(data, 4096)
    assert len(ranges) == 3 and [data[b:b + 3] for b, _ in ranges] == [b">s1", b">s2", b">s5"]
    fa = tmp_path / "long.fa"
    fa.write_bytes(data)
    dbs = {}
    for tag, env in (("host", {"MCQ_BUILD_PARSE_DEVICE": None}), ("one", {}), ("cut", {"MCQ_BUILD_PARSE_PIECE": "4096"})):
        db = str(tmp_path / tag)
        r = run("build", [db, str(fa)], env)
        if tag != "host":
            m = LINE.search(r.stderr)
            assert m and (int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(7)), int(m.group(8))) == (len(data), 6, 5, 1, 0), (tag, r.stderr[-1500:])
            assert int(m.group(1)) == (1 if tag == "one" else 2 * len(ranges)), (tag, m.group(0))        # cut: every range judged, then every range added
        dbs[tag] = parse_db(db)
    assert [dbs["host"]["taxa"][str(-t - 1)][4] for t in range(5)] == [0, 1, 3, 4, 5]      # the record numbers inside the file
    same_db(dbs["one"], dbs["host"], "one piece")
    same_db(dbs["cut"], dbs["host"], "cut")


def test_a_fastq_file_among_the_genomes_goes_to_the_host_loop(tmp_path):
    genomes = tmp_path / "genomes"
    shutil.copytree(os.path.join(GOLD, "build_in", "genomes"), genomes)
    (genomes / "reads_by_mistake.fq").write_bytes(b"@r1\nACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT\n+\n" + b"I" * 44 + b"\n")
    args = [str(genomes), "-taxonomy", "build_in/taxonomy"]
    runs = {}
    for tag, env in (("unset", {"MCQ_BUILD_PARSE_DEVICE": None, "MCQ_PROFILE": None}), ("set", {})):
        db = str(tmp_path / tag)
        r = run("build", [db] + args, env)
        runs[tag] = (parse_db(db), r.stdout, r.stderr)
    m = LINE.search(runs["set"][2])
    assert m and "reads_by_mistake.fq: FASTQ" in m.group(9) and int(m.group(7)) == 3, runs["set"][2][-1500:]
    assert "mcq profile" not in runs["unset"][2] and "parsed on the" not in runs["unset"][2]
    same_db(runs["set"][0], runs["unset"][0], "fastq among the genomes")
    strip = lambda s: re.sub(r"\d[\d.e+-]* s\b", "_ s", s).replace(str(tmp_path / "set"), "DB").replace(str(tmp_path / "unset"), "DB")
    assert strip(runs["set"][1]) == strip(runs["unset"][1])                    # stdout: the same lines but for the clock


def test_a_file_whose_sequences_need_more_room_than_its_bytes(tmp_path):
    """an empty header, no final newline and len % 4 == 1 at the file's end: seq takes one byte more than the file holds.  As a gathered
    piece and as the last range of a cut file the device path adds it; the database is the host loop's"""
    import numpy as np
    rng = np.random.default_rng(4)
    dna = lambda n: np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()
    fa = tmp_path / "tight.fa"
    fa.write_bytes(b">lead one\n" + dna(6000) + b"\n>\n" + dna(1001))
    alone = tmp_path / "alone.fa"
    alone.write_bytes(b">\n" + dna(2001))
    dbs = {}
    for tag, env in (("host", {"MCQ_BUILD_PARSE_DEVICE": None}), ("one", {}), ("cut", {"MCQ_BUILD_PARSE_PIECE": "4096"})):
        db = str(tmp_path / tag)
        r = run("build", [db, str(fa), str(alone)], env)
        if tag != "host":
            m = LINE.search(r.stderr)
            assert m and (int(m.group(3)), int(m.group(4)), int(m.group(7)), int(m.group(8))) == (3, 3, 2, 0), (tag, r.stderr[-1500:])
        dbs[tag] = parse_db(db)
    assert dbs["host"]["targets"] == 3
    same_db(dbs["one"], dbs["host"], "one piece")
    same_db(dbs["cut"], dbs["host"], "cut")
