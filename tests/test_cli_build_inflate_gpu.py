"""`mcq build` with MCQ_BUILD_INFLATE_DEVICE=1 beside MCQ_BUILD_PARSE_DEVICE=1 (TargetParseStep, mcq_build.h): the gzip files
among the genomes join their piece as compressed bytes and mc_inflate_streams writes them where mc_parse_targets reads.  The input is
tests/golden/build_in/genomes, which holds more.fa.gz, and a generated set of small .fa.gz files mixed with plain ones, with one file of
two members, one with FHCRC and one above a lowered MCQ_BUILD_INFLATE_MAX_MB: those three go to the host loop, each named with its
reason, and the database files are byte for byte those of the run with both switches unset.  MCQ_BUILD_INFLATE_DEVICE=1 alone changes
nothing but one line on stderr."""
import os
import re
import shutil
import subprocess

import pytest

import gzip_cases
from metacache_amd import build
from test_cli_build_gpu import GOLD, parse_db, same_db

pytestmark = pytest.mark.gpu
LINE = re.compile(r"^mcq profile: gzip references inflated on the device: (\d+) files, (\d+) bytes in, (\d+) bytes out, (\d+) mc_inflate_streams calls, kernels (\S+) ms, "
                  r"(\d+) gzip files left to the host(?: \((.*)\))?$", re.M)
ALONE = "mcq: MCQ_BUILD_INFLATE_DEVICE=1 has no effect without MCQ_BUILD_PARSE_DEVICE=1\n"


def run(args, env_extra):
    env = dict(os.environ)
    for k in ("MCQ_BUILD_PARSE_DEVICE", "MCQ_BUILD_INFLATE_DEVICE", "MCQ_BUILD_INFLATE_MAX_MB", "MCQ_BUILD_PARSE_PIECE", "MCQ_PROFILE"):
        env.pop(k, None)
    env.update(env_extra)
    r = subprocess.run([build.MCQ, "build"] + args, cwd=GOLD, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr
    return r


def db_files(prefix):
    """the files `build` wrote for the database `prefix`: name behind the prefix -> bytes"""
    d, base = os.path.split(prefix)
    out = {}
    for f in sorted(os.listdir(d)):
        if f.startswith(base) and os.path.isfile(os.path.join(d, f)):
            with open(os.path.join(d, f), "rb") as fh:
                out[f[len(base):]] = fh.read()
    assert out, prefix
    return out


@pytest.fixture(scope="module")
def genomes(tmp_path_factory):
    """-> (directory, {file: bytes in, bytes out} of the gzip files the device must take, {file: reason} of those it must leave)"""
    d = tmp_path_factory.mktemp("inflate_genomes") / "genomes"
    shutil.copytree(os.path.join(GOLD, "build_in", "genomes"), d)
    taken, left = {}, {}
    with open(d / "more.fa.gz", "rb") as f:
        z = f.read()
    import gzip
    taken["more.fa.gz"] = (len(z), len(gzip.decompress(z)))
    for i in range(24):
        text = gzip_cases.fasta_text(3000 + 517 * i, 100 + i)
        if i % 4 == 3:
            (d / ("gen_%02d.fa" % i)).write_bytes(text)
            continue
        z = gzip_cases.gz(text, level=(1, 6, 9)[i % 3], name=b"gen_%02d.fa" % i if i % 2 else None)
        (d / ("gen_%02d.fa.gz" % i)).write_bytes(z)
        taken["gen_%02d.fa.gz" % i] = (len(z), len(text))
    a, b = gzip_cases.fasta_text(5000, 201), gzip_cases.fasta_text(7000, 202)
    (d / "gen_chained.fa.gz").write_bytes(gzip_cases.gz(a) + gzip_cases.gz(b))
    left["gen_chained.fa.gz"] = "gzip: more bytes than its trailing size"      # the trailing ISIZE of a chain is its last member's: stated
    (d / "gen_fhcrc.fa.gz").write_bytes(gzip_cases.gz(gzip_cases.fasta_text(4000, 203), hcrc=True))
    left["gen_fhcrc.fa.gz"] = "gzip: header"
    (d / "gen_large.fa.gz").write_bytes(gzip_cases.gz(gzip_cases.fasta_text((1 << 20) + 5000, 204, repeats=True)))
    left["gen_large.fa.gz"] = "gzip: larger than MCQ_BUILD_INFLATE_MAX_MB"
    return str(d), taken, left


def test_gzip_genomes_on_the_device_write_the_same_database(genomes, tmp_path):
    d, taken, left = genomes
    args = [d, "-taxonomy", "build_in/taxonomy"]
    unset = run([str(tmp_path / "unset")] + args, {})
    both = run([str(tmp_path / "both")] + args, {"MCQ_BUILD_PARSE_DEVICE": "1", "MCQ_BUILD_INFLATE_DEVICE": "1", "MCQ_BUILD_INFLATE_MAX_MB": "1", "MCQ_PROFILE": "1"})
    m = LINE.search(both.stderr)
    assert m, both.stderr[-3000:]
    files, bytes_in, bytes_out, calls, ms, nleft, listed = m.groups()
    assert int(files) == len(taken) and int(bytes_in) == sum(v[0] for v in taken.values()) and int(bytes_out) == sum(v[1] for v in taken.values()), m.group(0)
    assert int(calls) >= 1 and float(ms) > 0 and int(nleft) == 3, m.group(0)
    reasons = {os.path.basename(x.split(": ", 1)[0]): x.split(": ", 1)[1] for x in listed.split("; ")}
    assert reasons == left, listed
    for name, why in left.items():                                             # the parse step's own lines name them too
        assert name + ": " + why in both.stderr
    a, b = db_files(str(tmp_path / "unset")), db_files(str(tmp_path / "both"))
    assert sorted(a) == sorted(b) and all(a[k] == b[k] for k in a), [k for k in a if a.get(k) != b.get(k)]
    same_db(parse_db(str(tmp_path / "both")), parse_db(str(tmp_path / "unset")), "both switches")
    assert "mcq profile" not in unset.stderr


def test_the_inflate_switch_alone_says_so_and_changes_nothing_else(genomes, tmp_path):
    d, _, _ = genomes
    args = [d, "-taxonomy", "build_in/taxonomy"]
    unset = run([str(tmp_path / "unset")] + args, {})
    alone = run([str(tmp_path / "alone")] + args, {"MCQ_BUILD_INFLATE_DEVICE": "1"})
    assert alone.stderr.count(ALONE) == 1 and alone.stderr.replace(ALONE, "") == unset.stderr
    strip = lambda s: re.sub(r"\d[\d.e+-]* s\b", "_ s", s).replace(str(tmp_path / "alone"), "DB").replace(str(tmp_path / "unset"), "DB")
    assert strip(alone.stdout) == strip(unset.stdout)
    a, b = db_files(str(tmp_path / "unset")), db_files(str(tmp_path / "alone"))
    assert sorted(a) == sorted(b) and all(a[k] == b[k] for k in a)
    silent = run([str(tmp_path / "silent")] + args + ["-silent"], {"MCQ_BUILD_INFLATE_DEVICE": "1"})
    assert ALONE not in silent.stderr
    # the parse switch without the inflate switch leaves every gzip file to the host with the reason it always had
    parse_only = run([str(tmp_path / "parse")] + args, {"MCQ_BUILD_PARSE_DEVICE": "1", "MCQ_PROFILE": "1"})
    assert "more.fa.gz: gzip;" in parse_only.stderr.replace(")", ";") and "inflated on the device" not in parse_only.stderr
