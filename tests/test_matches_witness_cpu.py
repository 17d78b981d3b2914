"""CPU: the model of the all-hits column (tests/matches_ref.py) and api.match_texts against the reference's own output, and the argument
checks of mc_format_matches* / mc_format_mappings_with that need no device.

The model is what tests/test_gpu_matches.py holds the device to.  Here it is itself held to the reference, on the reference's own lines
(tests/golden/cli_expected.json.gz, the reference CLI's output for toy32): the four golden command lines with -allhits.  Every read of
their input files goes through the C oracle (location list and top candidates), tests/classify_ref.py votes, and the model -- given that
list, those candidates, that assignment and the string tables of api.mapping_texts / api.match_texts -- must print the read's all-hits
column and its whole line again byte for byte."""
import ctypes as C
import gzip
import json
import os

import numpy as np
import pytest

import classify_ref
import cpuref
import format_ref
import matches_ref
from metacache_amd import api

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MC_OK, MC_ERR_INVALID, MC_ERR_NOMEM, MC_ERR_STATE = 0, -1, -3, -6
NUM_RANKS = 21
COLUMN = "\t|\t"
HIGHEST = 19                             # the command line's default of -highest: domain

# case -> (input files, reads that have a line, model flags, -lowest, keywords of mapping_texts).  reference_test_matrix: -allhits makes the
# reference print every read, -mapped-only or not (options.cpp sets the map view to "all" for it), so the model has no MAPPED_ONLY there.
CASES = {"everything_species": (["cli_reads.fa"], 399, format_ref.QUERY_IDS | format_ref.TOPHITS, 4, {"lowest": 4, "lineage": True, "taxids": True}),
         "allhits_sequence": (["cli_reads.fa"], 399, format_ref.TOPHITS, 0, {}),
         "pairfiles": (["cli_p1.fa", "cli_p2.fa"], 120, format_ref.QUERY_IDS | format_ref.TOPHITS, 0, {}),
         "reference_test_matrix": (["cli_truth.fa"], 300, format_ref.TRUTH | format_ref.TOPHITS, 0, {})}


def cli_case(name):
    with gzip.open(os.path.join(GOLDEN, "cli_expected.json.gz"), "rt") as f:
        return json.load(f)[name]


def header_number(lines, prefix):
    for l in lines:
        if l.startswith(prefix):
            return int(l[len(prefix):].split()[0])
    raise AssertionError(f"no '{prefix}' line")


def read_fasta(name):
    """-> [(name up to the first blank, sequence, query id)]; a record without a sequence has an id and no line"""
    recs = []
    with open(os.path.join(GOLDEN, name), "rb") as f:
        for line in f.read().split(b"\n"):
            if line.startswith(b">"):
                recs.append([line[1:].split(b" ")[0], b""])
            elif line.strip():
                recs[-1][1] += line.strip()
    return [(h, s, i + 1) for i, (h, s) in enumerate(recs) if s]


@pytest.fixture(scope="module")
def meta():
    """a metadata-only context of toy32 (no device): taxa as (id, parent, rank, name), taxon_lin[taxa, 21], target_lin[targets, 21]"""
    L = api.lib()
    h = C.c_void_p()
    assert L.mc_open_metadata(os.path.join(GOLDEN, "toy32").encode(), C.byref(h)) == MC_OK
    db = api.Database.from_handle(h.value, api.default_config())
    out = db.taxa(), db.taxon_table()[0], db.lineages()
    L.mc_destroy(h)
    return out


@pytest.fixture(scope="module")
def oracle_db():
    db = cpuref.oracle().open(os.path.join(GOLDEN, "toy32"))
    yield db
    db.close()


@pytest.mark.parametrize("case", sorted(CASES))
def test_model_prints_every_all_hits_column_and_line_of_the_reference_again(meta, oracle_db, case):
    taxa, taxon_lin, target_lin = meta
    files, want_lines, flags, lowest, text_kw = CASES[case]
    rec = cli_case(case)
    assert "-allhits" in rec["args"] and sorted(rec["files"]) == files
    hitmin = header_number(rec["lines"], "# Classification hit threshold is ")
    maxcand = header_number(rec["lines"], "# At maximum ")
    texts = api.mapping_texts(taxa, taxon_lin, target_lin, **text_kw)
    match_text = api.match_texts(taxa, target_lin, lowest)
    reads = read_fasta(files[0])
    mates = read_fasta(files[1]) if len(files) == 2 else None
    name_at = 1 if flags & format_ref.QUERY_IDS else 0
    # the reference's mapping lines, in read order (names repeat in cli_truth.fa): the body up to the tables that -abundances prints behind them
    ncols = 4 + (1 if flags & format_ref.QUERY_IDS else 0) + (1 if flags & format_ref.TRUTH else 0)
    body = [l for l in rec["lines"] if l and not l.startswith("#")]
    golden = body[:next((i for i, l in enumerate(body) if len(l.split(COLUMN)) != ncols), len(body))]
    assert len(golden) == want_lines
    nxt = 0
    result_index = {}
    for x, t in enumerate(texts[api.TEXT_RESULT]):
        result_index.setdefault(t.decode(), x)
    got_lines, columns_checked, wrong = [], 0, []
    for k, (name, seq, qid) in enumerate(reads):
        mate = b""
        if mates is not None:
            assert mates[k][0] == name
            mate = mates[k][1]
        hits, tops = oracle_db.query(seq, mate, max_cand=maxcand, lowest=lowest)
        row = np.zeros(maxcand, dtype=api.cand_dtype)
        for f in ("tgt", "hits", "beg", "end"):
            row[f][:len(tops)] = tops[f]
        taxon, rank, _ = classify_ref.vote(target_lin, row["tgt"], row["hits"], hitmin, api.hitdiff_factor(1.0), lowest, HIGHEST)
        column = matches_ref.piece(hits, match_text, windows=lowest == 0)
        want = None
        if not ((flags & format_ref.MAPPED_ONLY) and taxon == 0) and nxt < len(golden):
            want, nxt = golden[nxt], nxt + 1
        truth = 0
        if want is not None:
            cols = want.split(COLUMN)
            assert cols[name_at].encode() == name
            at = name_at + 1
            if flags & format_ref.TRUTH:
                truth = result_index[cols[at]]
                at += 1
            columns_checked += 1
            if cols[at].encode() != column:
                wrong.append((name, "column", cols[at][:200], column[:200]))
        got = matches_ref.line(k, extra=column, column=COLUMN.encode(), flags=flags, cands=row, taxon=taxon, rank=rank, name=name, query_id=qid, truth=truth,
                               result=texts[api.TEXT_RESULT], target_result=texts[api.TEXT_TARGET_RESULT], cand_text=texts[api.TEXT_CANDIDATE])
        if got != ((want + "\n").encode() if want is not None else b""):
            wrong.append((name, "line", want and want[-200:], got[-200:]))
        got_lines.append(got)
    assert not wrong, f"{len(wrong)} differences, first: {wrong[0]}"
    assert columns_checked == nxt == want_lines                          # every line of the reference was covered, none left out
    assert b"".join(got_lines) == "".join(l + "\n" for l in golden).encode()
    assert any(b"," in l for l in got_lines)


def test_model_without_the_column_is_the_model_of_the_lines():
    rng = np.random.default_rng(3)
    result = [b"--", b"a", b"bb"]
    for flags in (0, format_ref.QUERY_IDS | format_ref.TRUTH | format_ref.TOPHITS | format_ref.LOCATIONS, format_ref.MAPPED_ONLY):
        row = np.zeros(2, dtype=api.cand_dtype)
        row["tgt"], row["hits"] = [1, 0], [3, 2]
        kw = dict(column=b"\t", flags=flags, cands=row, taxon=int(rng.integers(0, 3)), rank=4, name=b"r", result=result, cand_text=[b"x", b"y"], truth=1, query_id=7)
        assert matches_ref.line(0, extra=None, **kw) == format_ref.line(0, **kw)
        with_column = matches_ref.line(0, extra=b"", **kw)
        assert with_column == b"" or len(with_column) == len(format_ref.line(0, **kw)) + 1


def test_model_rules():
    loc = lambda pairs: np.array([(w, t) for t, w in pairs], dtype=api.loc_dtype)
    texts = [b"A", b"", b"CC"]
    hits = loc([(0, 5), (0, 5), (0, 6), (1, 6), (2, 2 ** 31), (2, 2 ** 32 - 1), (3, 1), (3, 1), (0, 5)])
    tally = [0, 0]
    assert matches_ref.piece(hits, texts, True, tally) == b"A/5:2,A/6:1,CC/-2147483648:1,CC/-1:1,A/5:1," and tally == [5, 1]
    tally = [0, 0]
    assert matches_ref.piece(hits, texts, False, tally) == b"A:2,A:1,:1,CC:1,CC:1,A:1," and tally == [6, 1]
    assert matches_ref.piece(hits[:0], texts, True) == b"" and matches_ref.piece(hits, [], True) == b""


def test_match_texts_follow_the_host_rule(meta):
    taxa, _, target_lin = meta
    seq = api.match_texts(taxa, target_lin, 0)
    assert seq == [taxa[int(row[0]) - 1][3].encode() if row[0] else b"" for row in target_lin]
    species = api.match_texts(taxa, target_lin, 4)
    for t, row in enumerate(target_lin):
        x = int(row[4]) or int(row[0])
        assert species[t] == (taxa[x - 1][3].encode() if x else b"")
    assert species != seq


# ---- the C ABI without a device -------------------------------------------------------------------------------------------------
def test_new_names_are_exported():
    L = C.CDLL(api._build.build_library())
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "metacache_amd.h")).read()
    for n in ("mc_format_matches_set_text", "mc_format_matches", "mc_format_mappings_with", "mc_format_matches_stats"):
        assert hasattr(L, n) and n in api.EXPORTS and ("int " + n + "(") in header
    assert api.MATCHES_WINDOWS == 2 and "#define MC_MATCHES_WINDOWS    2" in header


@pytest.fixture()
def ctx():
    L = api.lib()
    h = C.c_void_p()
    assert L.mc_open_metadata(os.path.join(GOLDEN, "toy32").encode(), C.byref(h)) == MC_OK
    yield L, h
    L.mc_destroy(h)


def test_matches_set_text_checks(ctx):
    L, h = ctx
    data = np.frombuffer(b"--abc", dtype=np.uint8)
    off = np.array([0, 2, 5], dtype=np.uint64)
    st = L.mc_format_matches_set_text
    assert st(None, data.ctypes.data, off.ctypes.data, 2) == MC_ERR_INVALID
    assert st(h, data.ctypes.data, None, 2) == MC_ERR_INVALID
    assert st(h, None, off.ctypes.data, 2) == MC_ERR_INVALID
    for bad in ([1, 2, 5], [0, 4, 3]):
        assert st(h, data.ctypes.data, np.array(bad, dtype=np.uint64).ctypes.data, 2) == MC_ERR_INVALID
    stats = np.full(5, 9, dtype=np.uint64)
    assert L.mc_format_matches_stats(None, stats.ctypes.data) == MC_ERR_INVALID and L.mc_format_matches_stats(h, None) == MC_ERR_INVALID
    assert L.mc_format_matches_stats(h, stats.ctypes.data) == MC_OK and not stats.any()
    assert st(h, data.ctypes.data, off.ctypes.data, 0) == MC_OK              # an empty table is one
    assert st(h, None, np.zeros(3, dtype=np.uint64).ctypes.data, 2) == MC_OK  # ... and so is one of empty strings
    assert st(h, data.ctypes.data, off.ctypes.data, 2) == MC_OK
    assert L.mc_format_set_text(h, 3, data.ctypes.data, off.ctypes.data, 2) == MC_ERR_INVALID      # the old call has no fourth table
    assert L.mc_format_matches_stats(h, stats.ctypes.data) == MC_OK and not stats.any()


def test_matches_error_order_arguments_first_then_state(ctx):
    L, h = ctx
    n = 4
    buf = np.zeros(32768 + 64, dtype=np.uint8)                     # one buffer, so that aligned and overlapping addresses can be named
    base = (buf.ctypes.data + 63) & ~63
    hits, hit_off, out, piece_off = (base + o for o in (0, 1024, 2048, 8192))
    assert 8192 + (n + 1 + api.FORMAT_SCRATCH) * 8 <= 32768
    np.frombuffer(buf, dtype=np.uint64, count=n + 1, offset=hit_off - buf.ctypes.data)[:] = [0, 3, 3, 10, 16]
    HOST, WIN = api.FORMAT_HOST, api.MATCHES_WINDOWS

    def call(c=h, hi=hits, ho=hit_off, n=n, flags=HOST, o=out, cap=1024, po=piece_off):
        return L.mc_format_matches(c, hi, ho, n, flags, o, cap, po, None)

    assert call(c=None) == MC_ERR_INVALID
    assert call(ho=None) == MC_ERR_INVALID and call(po=None) == MC_ERR_INVALID and call(po=None, n=0) == MC_ERR_INVALID
    assert call(o=None) == MC_ERR_INVALID and call(hi=None) == MC_ERR_INVALID
    assert call(flags=HOST | 4) == MC_ERR_INVALID and call(flags=HOST | 64) == MC_ERR_INVALID and call(flags=1 << 20) == MC_ERR_INVALID
    assert call(flags=HOST | WIN) != MC_ERR_INVALID
    # misaligned device arrays (host arrays may lie anywhere)
    for kw in ({"o": out + 8}, {"hi": hits + 4}, {"ho": hit_off + 4}, {"po": piece_off + 4}):
        assert call(flags=0, **kw) == MC_ERR_INVALID, kw
        assert call(flags=WIN, **kw) == MC_ERR_INVALID, kw
    assert call(o=out + 8) != MC_ERR_INVALID and call(po=piece_off + 4) != MC_ERR_INVALID
    # out overlapping an input or piece_off
    for kw in ({"o": hits}, {"o": hit_off, "cap": 16}, {"o": hit_off + 32, "cap": 16}, {"o": piece_off - 1008}, {"o": piece_off + 16000, "cap": 16}):
        assert call(flags=0, **kw) == MC_ERR_INVALID, kw
    assert call(o=hits + 64, cap=64) == MC_ERR_INVALID and call(o=piece_off) == MC_ERR_INVALID     # (host lists: 16 locations = 128 bytes)
    assert call(o=hits + 128, cap=64) == MC_ERR_STATE
    assert call(flags=0, o=piece_off + 32768 - 8192, cap=16) == MC_ERR_STATE                            # (behind a device piece_off's workspace)
    # a host hit_off that decreases
    np.frombuffer(buf, dtype=np.uint64, count=n + 1, offset=hit_off - buf.ctypes.data)[:] = [0, 3, 2, 10, 16]
    assert call() == MC_ERR_INVALID and call(flags=0) == MC_ERR_STATE
    np.frombuffer(buf, dtype=np.uint64, count=n + 1, offset=hit_off - buf.ctypes.data)[:] = [0, 3, 3, 10, 16]
    assert L.mc_last_error(h)
    # valid arguments: nothing to do is fine on host arrays; work needs the table and a device -- this context has neither
    po = np.frombuffer(buf, dtype=np.uint64, count=1, offset=piece_off - buf.ctypes.data)
    po[0] = 7
    assert call(n=0) == MC_OK and po[0] == 0 and call(n=0, hi=None, ho=None, o=None, cap=0) == MC_OK
    assert call() == MC_ERR_STATE and b"mc_format_matches_set_text" in L.mc_last_error(h)
    data = np.frombuffer(b"--", dtype=np.uint8)
    off = np.array([0, 2], dtype=np.uint64)
    assert L.mc_format_matches_set_text(h, data.ctypes.data, off.ctypes.data, 1) == MC_OK
    assert call() == MC_ERR_STATE and call(flags=0) == MC_ERR_STATE and call(flags=0, n=0) == MC_ERR_STATE
    assert b"device" in L.mc_last_error(h)
    # bad arguments win over the missing device
    assert call(flags=HOST | 8) == MC_ERR_INVALID


def test_mappings_with_checks_what_mappings_checks_and_its_two_arrays(ctx):
    L, h = ctx
    n, stride = 4, 2
    buf = np.zeros(32768 + 64, dtype=np.uint8)
    base = (buf.ctypes.data + 63) & ~63
    cands, assigned, name_off, extra_off, names, extra, out, line_off = (base + o for o in (0, 256, 448, 512, 1024, 1536, 2048, 8192))
    np.frombuffer(buf, dtype=np.uint64, count=n + 1, offset=extra_off - buf.ctypes.data)[:] = [0, 10, 10, 40, 100]
    good = api.format_options()
    HOST = api.FORMAT_HOST

    def call(ctx=h, opt=good, c=cands, a=assigned, no=name_off, n=n, flags=HOST, o=out, cap=1024, lo=line_off, x=extra, xo=extra_off):
        return L.mc_format_mappings_with(ctx, C.byref(opt) if opt is not None else None, c, stride, a, None, None, 0, names, no, n, flags, o, cap, lo, None, x, xo)

    assert call(ctx=None) == MC_ERR_INVALID and call(opt=None) == MC_ERR_INVALID and call(c=None) == MC_ERR_INVALID and call(lo=None) == MC_ERR_INVALID
    assert call(flags=HOST | 64) == MC_ERR_INVALID and call(flags=1 << 20) == MC_ERR_INVALID        # no new flag
    assert call(xo=None) == MC_ERR_INVALID                                                           # extra without extra_off
    assert call(flags=0, xo=extra_off + 4) == MC_ERR_INVALID                                         # a misaligned device extra_off
    assert call(flags=0, x=extra + 1) != MC_ERR_INVALID                                              # (the bytes may lie anywhere)
    for kw in ({"o": extra}, {"o": extra + 96, "cap": 16}, {"o": extra_off + 32, "cap": 8}):
        assert call(**kw) == MC_ERR_INVALID, kw
    assert call(flags=0, o=extra_off, cap=16) == MC_ERR_INVALID and call(flags=0, o=extra, cap=16) == MC_ERR_INVALID
    assert call(o=extra + 112, cap=16) == MC_ERR_STATE                                               # (behind the pieces' 100 bytes)
    np.frombuffer(buf, dtype=np.uint64, count=n + 1, offset=extra_off - buf.ctypes.data)[:] = [0, 10, 5, 40, 100]
    assert call(x=None, xo=None) == MC_ERR_STATE and b"MC_TEXT_RESULT" in L.mc_last_error(h) and b"mc_format_mappings_with" in L.mc_last_error(h)
    data = np.frombuffer(b"--", dtype=np.uint8)
    off = np.array([0, 2], dtype=np.uint64)
    assert L.mc_format_set_text(h, api.TEXT_RESULT, data.ctypes.data, off.ctypes.data, 1) == MC_OK
    assert call() == MC_ERR_STATE and b"device" in L.mc_last_error(h)
    assert call(n=0) == MC_OK and call(n=0, x=None, xo=None) == MC_OK
