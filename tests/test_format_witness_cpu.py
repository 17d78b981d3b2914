"""CPU: the model of the mapping lines (tests/format_ref.py) and api.mapping_texts against the reference's own output, and the argument
checks of mc_format_* that need no device.

The model is what tests/test_gpu_format.py holds the device to.  Here it is itself held to the reference, on the reference's own lines
(tests/golden/cli_expected.json.gz, the reference CLI's output for toy32): the lines of four golden cases carry the read's candidates in
their -tophits column at sequence level, so the candidates are parsed from the line, tests/classify_ref.py votes, and the model -- given
those candidates, that assignment and the string tables of api.mapping_texts -- must print the line again byte for byte.  Every line of
a case is checked.  The 144 outputs of `format_matrix` (every combination of the options that shape a taxon's text) are printed again from
the assignments that its plainest output names, and the truth column from the golden case `ground_truth`."""
import ctypes as C
import gzip
import json
import os

import numpy as np
import pytest

import classify_ref
import format_ref
from metacache_amd import api

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MC_OK, MC_ERR_INVALID, MC_ERR_NOMEM, MC_ERR_STATE = 0, -1, -3, -6
NUM_RANKS = 21
COLUMN = "\t|\t"
HIGHEST = 19                             # the command line's default of -highest: domain

# case -> (mapping lines it must have, -hitdiff, -maxcand, flags of the model)
TOPHITS_CASES = {"mapped_only_vote": (221, 0.5, 4, format_ref.TOPHITS | format_ref.MAPPED_ONLY),
                 "pairseq": (120, 1.0, 2, format_ref.TOPHITS | format_ref.QUERY_IDS),
                 "gzip_input": (399, 1.0, 2, format_ref.TOPHITS | format_ref.QUERY_IDS),
                 "fastq_irregular": (49, 1.0, 2, format_ref.TOPHITS | format_ref.QUERY_IDS)}


def cli_case(name):
    with gzip.open(os.path.join(GOLDEN, "cli_expected.json.gz"), "rt") as f:
        return json.load(f)[name]


def header_number(lines, prefix):
    for l in lines:
        if l.startswith(prefix):
            return int(l[len(prefix):].split()[0])
    raise AssertionError(f"no '{prefix}' line")


@pytest.fixture(scope="module")
def meta():
    """a metadata-only context of toy32 (no device): handle, taxa as (id, parent, rank, name), taxon_lin[taxa, 21], target_lin[targets, 21]"""
    L = api.lib()
    h = C.c_void_p()
    assert L.mc_open_metadata(os.path.join(GOLDEN, "toy32").encode(), C.byref(h)) == MC_OK
    db = api.Database.from_handle(h.value, api.default_config())
    taxa = db.taxa()
    taxon_lin = db.taxon_table()[0]
    target_lin = db.lineages()
    yield h, taxa, taxon_lin, target_lin
    L.mc_destroy(h)


def body_of(lines):
    return [l for l in lines if l and not l.startswith("#")]


@pytest.mark.parametrize("case", sorted(TOPHITS_CASES))
def test_model_prints_every_reference_line_again(meta, case):
    _, taxa, taxon_lin, target_lin = meta
    want_lines, hitdiff, maxcand, flags = TOPHITS_CASES[case]
    rec = cli_case(case)
    z = np.load(os.path.join(GOLDEN, "toy32_expected.npz"))
    tgt_of = {str(nm): t for t, nm in enumerate(z["target_names"])}
    hitmin = header_number(rec["lines"], "# Classification hit threshold is ")
    assert header_number(rec["lines"], "# At maximum ") == maxcand
    body = body_of(rec["lines"])
    assert len(body) == want_lines
    texts = api.mapping_texts(taxa, taxon_lin, target_lin)
    factor = api.hitdiff_factor(hitdiff)
    wrong = []
    for l in body:
        cols = l.split(COLUMN)
        qid, name = (int(cols[0]), cols[1]) if flags & format_ref.QUERY_IDS else (0, cols[0])
        ents = [e.rsplit(":", 1) for e in cols[-2].split(",") if e]
        row = np.zeros(max(maxcand, len(ents)), dtype=api.cand_dtype)
        for j, (nm, hits) in enumerate(ents):
            row[j]["tgt"], row[j]["hits"] = tgt_of[nm], int(hits)
        taxon, rank, _ = classify_ref.vote(target_lin, row["tgt"], row["hits"], hitmin, factor, 0, HIGHEST)
        got = format_ref.line(0, column=COLUMN.encode(), flags=flags, cands=row, taxon=taxon, rank=rank, name=name.encode(), query_id=qid,
                              result=texts[api.TEXT_RESULT], target_result=texts[api.TEXT_TARGET_RESULT], cand_text=texts[api.TEXT_CANDIDATE])
        if got != (l + "\n").encode():
            wrong.append((l, got))
    assert not wrong, f"{len(wrong)} of {len(body)} lines differ, first: {wrong[0]}"


def matrix_options(args):
    """the options of a format_matrix entry that shape a line -> (keywords of mapping_texts, model flags, column)"""
    kw = {"taxids": "-taxids" in args, "taxids_only": "-taxids-only" in args, "omit_ranks": "-omit-ranks" in args, "lineage": "-lineage" in args,
          "separate_cols": "-separate-cols" in args}
    column = args[args.index("-separator") + 1] if "-separator" in args else COLUMN
    flags = (format_ref.QUERY_IDS if "-queryids" in args else 0) | (format_ref.MAPPED_ONLY if "-mapped-only" in args else 0)
    known = {"-no-summary", "-no-query-params", "-taxids", "-taxids-only", "-omit-ranks", "-lineage", "-separate-cols", "-separator", "-queryids", "-mapped-only", column}
    assert set(args) <= known, args
    return kw, flags, column


def test_all_144_outputs_of_the_format_matrix(meta):
    _, taxa, taxon_lin, target_lin = meta
    fm = cli_case("format_matrix")
    assert len(fm["matrix"]) == 144 and len(fm["outputs"]) == 144
    index_of_id = {t[0]: i for i, t in enumerate(taxa)}
    # who was assigned what: the output that prints "rank:name(id)" and nothing else names every read's taxon by its id
    plain = fm["matrix"].index(["-no-summary", "-no-query-params", "-taxids"])
    names, assigned, first_tgt = [], [], []
    for l in body_of(fm["outputs"][plain]):
        name, verdict = l.split(COLUMN)
        names.append(name.encode())
        if verdict == "--":
            assigned.append((0, NUM_RANKS)); first_tgt.append(0)
            continue
        tid = int(verdict[verdict.rindex("(") + 1:-1])
        x = index_of_id[tid]
        assigned.append((x + 1, taxa[x][2]))
        first_tgt.append(-tid - 1 if tid < 0 else 0)                   # (a sequence-level result is its top candidate's target)
    assert len(names) == 30 and any(r == 0 for _, r in assigned) and any(0 < r < NUM_RANKS for _, r in assigned)
    for args, out in zip(fm["matrix"], fm["outputs"]):
        kw, flags, column = matrix_options(args)
        texts = api.mapping_texts(taxa, taxon_lin, target_lin, separator=column, **kw)
        got = []
        for i, name in enumerate(names):
            row = np.zeros(1, dtype=api.cand_dtype)
            row[0]["tgt"], row[0]["hits"] = first_tgt[i], 1
            got.append(format_ref.line(i, column=column.encode(), flags=flags, cands=row, taxon=assigned[i][0], rank=assigned[i][1], name=name,
                                       query_id=i + 1, result=texts[api.TEXT_RESULT], target_result=texts[api.TEXT_TARGET_RESULT]))
        want = "".join(l + "\n" for l in body_of(out)).encode()
        assert b"".join(got) == want, args
        # the same without the table of the targets: a target's taxon prints what the target prints
        again = b"".join(format_ref.line(i, column=column.encode(), flags=flags, cands=np.zeros(1, dtype=api.cand_dtype), taxon=assigned[i][0],
                                         rank=assigned[i][1], name=names[i], query_id=i + 1, result=texts[api.TEXT_RESULT]) for i in range(len(names)))
        assert again == want, args


def test_truth_column_of_the_ground_truth_case(meta):
    _, taxa, taxon_lin, target_lin = meta
    rec = cli_case("ground_truth")
    assert rec["args"] == ["-ground-truth", "-taxids"]
    index_of_id = {t[0]: i for i, t in enumerate(taxa)}
    texts = api.mapping_texts(taxa, taxon_lin, target_lin, taxids=True)

    def taxon_of(text):
        return 0 if text == "--" else index_of_id[int(text[text.rindex("(") + 1:-1])] + 1

    body = body_of(rec["lines"])
    assert len(body) == 300
    for l in body:
        name, truth, verdict = l.split(COLUMN)
        a = taxon_of(verdict)
        got = format_ref.line(0, column=COLUMN.encode(), flags=format_ref.TRUTH, cands=np.zeros(1, dtype=api.cand_dtype), taxon=a,
                              rank=taxa[a - 1][2] if a else NUM_RANKS, name=name.encode(), truth=taxon_of(truth), result=texts[api.TEXT_RESULT])
        assert got == (l + "\n").encode()


def test_lowest_rank_candidate_texts(meta):
    """-lowest species: a candidate prints the id of its target's taxon on that rank or the next one above (show_candidates), as the lines
    of the golden case hitdiff_percent do"""
    _, taxa, taxon_lin, target_lin = meta
    texts = api.mapping_texts(taxa, taxon_lin, target_lin, lowest=4)
    seen = {e.rsplit(":", 1)[0] for l in body_of(cli_case("hitdiff_percent")["lines"]) for e in l.split(COLUMN)[2].split(",") if e}
    assert seen and seen <= {t.decode() for t in texts[api.TEXT_CANDIDATE]}
    for t, row in enumerate(target_lin):
        x = next(int(v) for v in row[4:] if v)
        assert texts[api.TEXT_CANDIDATE][t] == str(taxa[x - 1][0]).encode()


# ---- the C ABI without a device -------------------------------------------------------------------------------------------------
def test_new_names_are_exported():
    L = C.CDLL(api._build.build_library())
    for n in ("mc_format_set_text", "mc_format_mappings", "mc_format_stats"):
        assert hasattr(L, n) and n in api.EXPORTS
    assert C.sizeof(api.McFormatOptions) == 28


def test_set_text_checks():
    L = api.lib()
    h = C.c_void_p()
    assert L.mc_open_metadata(os.path.join(GOLDEN, "toy32").encode(), C.byref(h)) == MC_OK
    try:
        data = np.frombuffer(b"--abc", dtype=np.uint8)
        off = np.array([0, 2, 5], dtype=np.uint64)
        st = L.mc_format_set_text
        assert st(None, api.TEXT_RESULT, data.ctypes.data, off.ctypes.data, 2) == MC_ERR_INVALID
        assert st(h, 3, data.ctypes.data, off.ctypes.data, 2) == MC_ERR_INVALID and st(h, -1, data.ctypes.data, off.ctypes.data, 2) == MC_ERR_INVALID
        assert st(h, api.TEXT_RESULT, data.ctypes.data, None, 2) == MC_ERR_INVALID
        assert st(h, api.TEXT_RESULT, None, off.ctypes.data, 2) == MC_ERR_INVALID
        assert st(h, api.TEXT_RESULT, data.ctypes.data, off.ctypes.data, 0) == MC_ERR_INVALID          # no entry 0
        assert st(h, api.TEXT_CANDIDATE, data.ctypes.data, off.ctypes.data, 0) == MC_OK                 # an empty table of targets is one
        bad = np.array([1, 2, 5], dtype=np.uint64)
        assert st(h, api.TEXT_RESULT, data.ctypes.data, bad.ctypes.data, 2) == MC_ERR_INVALID
        bad = np.array([0, 4, 3], dtype=np.uint64)
        assert st(h, api.TEXT_RESULT, data.ctypes.data, bad.ctypes.data, 2) == MC_ERR_INVALID
        assert st(h, api.TEXT_RESULT, data.ctypes.data, off.ctypes.data, 2) == MC_OK
        stats = np.full(5, 9, dtype=np.uint64)
        assert L.mc_format_stats(None, stats.ctypes.data) == MC_ERR_INVALID and L.mc_format_stats(h, None) == MC_ERR_INVALID
        assert L.mc_format_stats(h, stats.ctypes.data) == MC_OK and not stats.any()
    finally:
        L.mc_destroy(h)


def test_error_order_arguments_first_then_state():
    L = api.lib()
    h = C.c_void_p()
    assert L.mc_open_metadata(os.path.join(GOLDEN, "toy32").encode(), C.byref(h)) == MC_OK
    try:
        n, stride = 4, 2
        buf = np.zeros(32768 + 64, dtype=np.uint8)                 # one buffer, so that aligned and overlapping addresses can be named
        base = (buf.ctypes.data + 63) & ~63
        # (a device line_off reaches n + 1 + MC_FORMAT_SCRATCH entries far: it comes last)
        cands, assigned, truth, ids, name_off, names, out, line_off = (base + o for o in (0, 256, 320, 384, 448, 1024, 2048, 8192))
        assert 8192 + (n + 1 + api.FORMAT_SCRATCH) * 8 <= 32768
        good = api.format_options()
        HOST = api.FORMAT_HOST

        def call(ctx=h, opt=good, c=cands, stride=stride, a=assigned, t=None, q=None, nm=names, no=name_off, n=n, flags=HOST, o=out, cap=1024, lo=line_off):
            return L.mc_format_mappings(ctx, C.byref(opt) if opt is not None else None, c, stride, a, t, q, 0, nm, no, n, flags, o, cap, lo, None)

        # NULL where needed
        assert call(ctx=None) == MC_ERR_INVALID
        assert call(opt=None) == MC_ERR_INVALID
        assert call(c=None) == MC_ERR_INVALID and call(a=None) == MC_ERR_INVALID and call(no=None) == MC_ERR_INVALID
        assert call(lo=None) == MC_ERR_INVALID and call(lo=None, n=0) == MC_ERR_INVALID
        assert call(o=None) == MC_ERR_INVALID
        assert call(stride=0) == MC_ERR_INVALID and call(stride=0, n=0) == MC_ERR_INVALID
        long_column = api.format_options(column=b"x" * 17)
        assert long_column.column_len == 17 and call(opt=long_column) == MC_ERR_INVALID
        assert call(opt=api.format_options(column=b"x" * 16)) != MC_ERR_INVALID
        assert call(flags=HOST | 64) == MC_ERR_INVALID and call(flags=1 << 20) == MC_ERR_INVALID
        assert call(flags=HOST | api.FORMAT_TRUTH) == MC_ERR_INVALID                     # MC_FORMAT_TRUTH without truth
        assert call(flags=HOST | api.FORMAT_TRUTH, t=truth) != MC_ERR_INVALID
        # misaligned device arrays (host arrays may lie anywhere)
        for kw in ({"o": out + 8}, {"c": cands + 8}, {"a": assigned + 4}, {"q": ids + 4}, {"no": name_off + 4}, {"lo": line_off + 4}, {"t": truth + 2}):
            assert call(flags=0, **kw) == MC_ERR_INVALID, kw
            assert call(flags=HOST, **kw) != MC_ERR_INVALID, kw
        # out overlapping an input
        for kw in ({"o": cands}, {"o": cands + 112, "cap": 16}, {"o": assigned - 16}, {"o": names, "cap": 16}, {"o": line_off - 1008}, {"o": line_off + 16000, "cap": 16},
                   {"o": name_off}, {"o": truth - 64, "t": truth}, {"o": ids, "q": ids, "cap": 16}):
            assert call(flags=0, **kw) == MC_ERR_INVALID, kw
        assert call(flags=0, o=ids, cap=16) == MC_ERR_STATE                              # (no id array: those bytes are nobody's)
        assert call(o=line_off) == MC_ERR_INVALID
        assert L.mc_last_error(h)
        # valid arguments: nothing to do is fine on host arrays; work needs the tables and a device -- this context has neither
        assert call(n=0) == MC_OK and call(n=0, c=None, a=None, no=None, nm=None, o=None, cap=0) == MC_OK
        assert call() == MC_ERR_STATE and b"MC_TEXT_RESULT" in L.mc_last_error(h)
        data = np.frombuffer(b"--", dtype=np.uint8)
        off = np.array([0, 2], dtype=np.uint64)
        assert L.mc_format_set_text(h, api.TEXT_RESULT, data.ctypes.data, off.ctypes.data, 1) == MC_OK
        assert call(flags=HOST | api.FORMAT_TOPHITS) == MC_ERR_STATE and b"MC_TEXT_CANDIDATE" in L.mc_last_error(h)
        assert L.mc_format_set_text(h, api.TEXT_CANDIDATE, data.ctypes.data, off.ctypes.data, 1) == MC_OK
        assert call(flags=HOST | api.FORMAT_TOPHITS) == MC_ERR_STATE and call(flags=0) == MC_ERR_STATE and call(flags=0, n=0) == MC_ERR_STATE
        assert b"device" in L.mc_last_error(h)
        # bad arguments win over the missing device
        assert call(stride=0) == MC_ERR_INVALID
    finally:
        L.mc_destroy(h)
