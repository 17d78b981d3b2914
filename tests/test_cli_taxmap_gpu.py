"""`mcq build` / `modify` / `build+query` with MCQ_TAXMAP_DEVICE=1 (TaxmapStep, mcq_build.h): the ranking pass over the accession2taxid
tables runs in the library (mc_taxmap_*).  The golden cases default, u16, reset_taxa, modify_default and bq_default give the taxa -- every
target's parent among them -- and the query lines of the reference; stderr names the device step with 0 files left to the host.  A copy of
the table with a '\\r' in it is refused by the device: the host loop ranks (the same taxa) and mcq says so with file, verdict and offence."""
import os
import shutil
import subprocess

import pytest

from metacache_amd import build
from test_cli_build_gpu import EXP, GOLD, parse_db, same_db
from test_cli_gpu import _same

pytestmark = pytest.mark.gpu
DEVICE_LINE = "mcq profile: targets ranked on the device: "


def mcq(args, **env):
    e = dict(os.environ, MCQ_TAXMAP_DEVICE="1", MCQ_PROFILE="1")
    e.update(env)
    r = subprocess.run([build.MCQ] + args, cwd=GOLD, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r


def device_line(r):
    lines = [l for l in r.stderr.split("\n") if l.startswith(DEVICE_LINE)]
    assert len(lines) == 1 and lines[0].endswith(", 0 files left to the host") and "ranked on the host" not in r.stderr, r.stderr
    return lines[0]


@pytest.mark.parametrize("case", ["default", "u16", "reset_taxa"])
def test_build_ranks_on_the_device(case, tmp_path):
    build.build_library()
    c = EXP["build"][case]
    db = str(tmp_path / case)
    r = mcq(["build", db] + c["args"] + c["mcq_extra"])
    line = device_line(r)
    assert " 1 mc_taxmap_add calls, " in line and " 4 rows, " in line and " 1 files, " in line, line   # (one target has no row, so the whole table is read: one piece)
    same_db(parse_db(db), c["db"], case)
    assert "Try to map sequences to taxa using 'build_in/taxonomy/toy.accession2taxid'" in r.stdout


def test_build_ranks_in_pieces(tmp_path):
    """MCQ_TAXMAP_PIECE=40: every row of the toy table is a call of its own"""
    build.build_library()
    c = EXP["build"]["reset_taxa"]
    db = str(tmp_path / "pieces")
    r = mcq(["build", db] + c["args"] + c["mcq_extra"], MCQ_TAXMAP_PIECE="40")
    assert " 4 mc_taxmap_add calls, " in device_line(r)
    same_db(parse_db(db), c["db"], "reset_taxa/pieces")


def test_modify_ranks_on_the_device(tmp_path):
    build.build_library()
    c = EXP["modify"]["modify_default"]
    db = str(tmp_path / "modify_default")
    for mode, args in (("build", c["first"] + c["mcq_extra"]), ("modify", c["second"])):
        device_line(mcq([mode, db] + args))
    same_db(parse_db(db), c["db"], "modify_default")


def test_build_query_ranks_on_the_device(tmp_path):
    build.build_library()
    c = EXP["bq"]["bq_default"]
    out = tmp_path / "bq.txt"
    r = mcq(["build+query"] + c["args"] + ["-threads", "1", "-out", str(out)])
    device_line(r)
    _same(out.read_text().split("\n"), c["lines"], "bq_default")


@pytest.mark.parametrize("silent", [False, True])
def test_a_refused_table_is_ranked_on_the_host(silent, tmp_path):
    build.build_library()
    c = EXP["build"]["default"]
    tax = tmp_path / "taxonomy"
    shutil.copytree(os.path.join(GOLD, "build_in", "taxonomy"), tax)
    table = tax / "toy.accession2taxid"
    data = table.read_bytes()
    third = data.index(b"\n", data.index(b"\n") + 1) + 1           # the start of the table's third line
    table.write_bytes(data[:third - 1] + b"\r" + data[third - 1:])
    args = [str(tax) if a == "build_in/taxonomy" else a for a in c["args"]]
    assert args != c["args"]
    db = str(tmp_path / "crlf")
    # -silent without MCQ_PROFILE is the only way to keep the fall-back quiet; with either it is said
    r = mcq(["build", db] + args + c["mcq_extra"] + (["-silent"] if silent else []))
    assert DEVICE_LINE not in r.stderr
    first = data.index(b"\n") + 1
    assert "mcq: targets ranked on the host (" + str(table) + ": verdict 1 (irregular line) at offset " + str(first) + ")" in r.stderr, r.stderr
    same_db(parse_db(db), c["db"], "default/crlf")
    if silent:
        e = dict(os.environ, MCQ_TAXMAP_DEVICE="1")
        e.pop("MCQ_PROFILE", None)
        q = subprocess.run([build.MCQ, "build", db + "_quiet"] + args + c["mcq_extra"] + ["-silent"], cwd=GOLD, env=e, capture_output=True, text=True, timeout=600)
        assert q.returncode == 0 and "ranked on the host" not in q.stderr
