"""CPU: the witness of mc_merge_results_* (merge_results_ref) against the reference's own `metacache merge`: driven with the golden part
files and the toy taxonomy its lists equal the top_hits column of the committed merge_expected.json.gz cases that print it, and its
assignments the taxid and rank of species_lineage's last column.  Then every generated input the device tests use: the witness accepts
the regular ones as regular and refuses each irregular one at the line the case names."""
import gzip
import json
import os

import pytest

import merge_results_cases as cases
import merge_results_ref as ref

with gzip.open(os.path.join(cases.GOLDEN, "merge_expected.json.gz"), "rt") as f:
    EXP = json.load(f)


@pytest.fixture(scope="module")
def toy():
    return cases.toy_table()


def merged(toy, files, max_cand, merge_below=4, capacity=700):
    ids, lin, rank, _ = toy
    m = ref.Merger(ids, lin, rank, capacity, max_cand, merge_below)
    datas = []
    for name in sorted(files):                                # merge sorts the file names
        data = cases.golden_part(os.path.basename(name))
        body = data[data.index(b"\n", data.index(b"# TABLE_LAYOUT")) + 1:]
        lines = sum(1 for l in body.split(b"\n") if l and not l.startswith(b"#"))
        st = m.add(body, cases.tophits_column(data), file_lines=lines)
        assert st[5] == ref.OK, (name, st)
        datas.append(body)
    return m, datas


def expected_rows(case):
    layout = next(l for l in EXP[case]["lines"] if l.startswith("# TABLE_LAYOUT:"))
    cols = [c.strip() for c in layout[15:].split("|")]
    rows = [[c.strip() for c in l.split("\t|\t")] for l in EXP[case]["lines"] if l and not l.startswith("#")]
    return cols, rows


def top_hits_text(m, ids, q):
    return ",".join(f"{int(ids[x - 1])}:{h}" for x, h in m.lists[q])


@pytest.mark.parametrize("case,max_cand", [("directory", 4), ("vote", 4), ("species_lineage", 3), ("genus", 2)])
def test_lists_equal_the_references_top_hits(toy, case, max_cand):
    ids = toy[0]
    files = ["part0.txt", "part1.txt"] if case == "directory" else EXP[case]["files"]
    lowest = 6 if case == "genus" else 4
    m, datas = merged(toy, files, max_cand, merge_below=lowest)
    cols, rows = expected_rows(case)
    hcol, tcol = cols.index("query_header"), cols.index("top_hits")
    by_header = {}
    for q in range(m.count):
        call, off, length = m.hdr[q]
        if length:
            by_header[datas[call][off:off + length].decode()] = q
    assert rows
    for row in rows:                                          # (-mapped-only prints a subset: every printed row is checked)
        if not row[hcol]:                                     # an id no file has a line for: no header, no hits
            assert row[tcol] == ""
            continue
        q = by_header[row[hcol]]
        assert top_hits_text(m, ids, q) == row[tcol], (case, row)
    if case != "vote":
        assert len(rows) == m.count


def test_assignments_equal_the_references_lineage_column(toy):
    ids = toy[0]
    m, datas = merged(toy, EXP["species_lineage"]["files"], 3)
    cols, rows = expected_rows("species_lineage")
    out = m.classify(5, 1.0, ref.NUM_RANKS - 2)               # merge: hitmin 5, hitdiff 1 (the factor), highest domain
    assert len(rows) == m.count
    for q, row in enumerate(rows):
        call, off, length = m.hdr[q]
        assert datas[call][off:off + length].decode() == row[0] if length else row[0] == ""
        first = row[-1].split(",")[0]                         # "rank:name(taxid)" of the lowest match, or "--"
        taxon, rank, _ = map(int, out[q])
        if first.startswith("--"):
            assert taxon == 0, (q, row[-1])
            continue
        name_rank = first.split(":")[0]
        taxid = int(first[first.rindex("(") + 1:-1])
        assert taxon and int(ids[taxon - 1]) == taxid and cases.RANK_NAMES[rank] == name_rank, (q, first, taxon, rank)


def test_generated_inputs_are_what_they_claim(toy):
    ids, lin, rank, _ = toy
    T = 4096
    for name, data in {**cases.generated_files(ids, rank), **cases.tile_files(T, ids, rank)}.items():
        lines, comments, offence, parsed = ref.judge(data, cases.COL)
        assert offence is None and len(parsed) == lines, (name, offence)
        assert len({p[1] for p in parsed}) == lines, name     # no query twice
    assert len(cases.tile_files(T, ids, rank)["many_tiles"]) > 256 * T
    for name, (data, at) in cases.irregular_files(ids, rank).items():
        m = ref.Merger(ids, lin, rank, 64, 4, 4)
        st = m.add(data, cases.COL)
        assert st[5] == ref.IRREGULAR and st[6] == at, (name, st)


def test_generated_files_hold_the_cases_they_are_made_for(toy):
    ids, lin, rank, _ = toy
    files = cases.generated_files(ids, rank)
    m = ref.Merger(ids, lin, rank, 64, 8, 4)
    sts = [m.add(files[k], cases.COL) for k in "abc"]
    assert [s[5] for s in sts] == [ref.OK] * 3
    assert sts[0][2] == 60 and sts[1][2] == 30 and sts[2][2] == 45     # the cut: file b's 29 lines end the 60 lists of file a
    assert all(s[4] >= 1 for s in sts)                                   # unknown taxids are counted
    assert m.lists[0] == [] and m.hdr[0][2] > 0                          # an empty list in every file keeps its header
    assert m.lists[57] == [] and m.hdr[57] == (0, 0, 0)                  # the query of file a alone was cut off
    assert (rank == ref.NUM_RANKS).any()                                 # the toy taxonomy has taxa without a rank (merged ids)
    unclassified_top = m.classify(5, 1.0, 19)[5]
    assert m.lists[5] and rank[m.lists[5][0][0] - 1] == ref.NUM_RANKS and unclassified_top[0] == 0


# ---- the generated part files: golden/merge_cases_in, expected lines made by the reference (make_golden_merge_cases.py) ---------------
with gzip.open(os.path.join(cases.GOLDEN, "merge_cases_expected.json.gz"), "rt") as f:
    CASES_EXP = json.load(f)


def arg_of(args, name, default):
    return args[args.index(name) + 1] if name in args else default


def test_committed_part_files_are_the_generated_ones(toy):
    ids, _, rank, _ = toy
    for name, data in cases.generated_files(ids, rank).items():
        with open(os.path.join(cases.GOLDEN, "merge_cases_in", name + ".txt"), "rb") as f:
            assert f.read() == data, name


@pytest.mark.parametrize("case", sorted(CASES_EXP))
def test_generated_cases_equal_the_reference(toy, case):
    ids, lin, rank, _ = toy
    c = CASES_EXP[case]
    args = c["args"]
    max_cand = int(arg_of(args, "-maxcand", 2))
    hitmin, hitdiff = int(arg_of(args, "-hitmin", 5)), float(arg_of(args, "-hitdiff", 1.0))
    highest = cases.RANK_NAMES.index(arg_of(args, "-highest", "domain"))
    m = ref.Merger(ids, lin, rank, 64, max_cand, 4)
    for name in sorted(c["files"]):
        with open(os.path.join(cases.GOLDEN, name), "rb") as f:
            data = f.read()
        st = m.add(data, cases.tophits_column(data))
        assert st[5] == ref.OK, (name, st)                                   # a case the line rule refuses proves nothing about the device
    out = m.classify(hitmin, hitdiff, highest)
    layout = next(l for l in c["lines"] if l.startswith("# TABLE_LAYOUT:"))
    cols = [x.strip() for x in layout[15:].split("|")]
    rows = [[x.strip() for x in l.split("\t|\t")] for l in c["lines"] if l and not l.startswith("#")]
    assert rows and (len(rows) == m.count or "-mapped-only" in args)
    for row in rows:
        q = int(row[0]) - 1
        assert top_hits_text(m, ids, q) == row[cols.index("top_hits")], (case, row)
        first = row[-1].split(",")[0]
        taxon, r, _ = map(int, out[q])
        if first.startswith("--"):
            assert taxon == 0, (case, row)
        else:
            assert taxon and int(ids[taxon - 1]) == int(first[first.rindex("(") + 1:-1]) and cases.RANK_NAMES[r] == first.split(":")[0], (case, row)
    if "-mapped-only" in args:
        assert len(rows) == int((out[:m.count, 0] != 0).sum())
