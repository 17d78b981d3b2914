"""CPU: the numpy model of the ranked-LCA vote (tests/classify_ref.py) against the reference's own mapping lines, and the argument
checks of mc_classify_candidates / mc_classify_tally that need no device.

The model is what tests/test_gpu_classify.py holds the device to.  Here it is itself held to the reference: every mapping line of three
golden cases (tests/golden/cli_expected.json.gz, the reference CLI's output for toy32) carries the read's candidates in its -tophits
column and the reference's verdict in its last column; the model, given those candidates and the lineages of
tests/golden/toy32_expected.npz, must arrive at the same rank and the same taxon on every line."""
import ctypes as C
import gzip
import json
import os

import numpy as np
import pytest

import classify_ref
from cpuref import RANKS
from metacache_amd import api

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MC_OK, MC_ERR_INVALID, MC_ERR_STATE = 0, -1, -6

# case -> (mapping lines it must have, -hitdiff, -maxcand: 0 = unlimited)
WITNESS_CASES = {"allhits_sequence": (399, 1.0, 3), "mapped_only_vote": (221, 0.5, 4), "maxcand_unlimited_seq": (639, 1.0, 0)}


def cli_case(name):
    with gzip.open(os.path.join(GOLDEN, "cli_expected.json.gz"), "rt") as f:
        return json.load(f)[name]


def header_number(lines, prefix):
    for l in lines:
        if l.startswith(prefix):
            return int(l[len(prefix):].split()[0])
    raise AssertionError(f"no '{prefix}' line")


def metadata_taxa():
    """(taxon id, name) of every taxon of toy32, from its .meta file (no device needed)"""
    L = api.lib()
    h = C.c_void_p()
    assert L.mc_open_metadata(os.path.join(GOLDEN, "toy32").encode(), C.byref(h)) == MC_OK
    try:
        n = C.c_uint64()
        assert L.mc_db_num_taxa(h, C.byref(n)) == MC_OK
        out = []
        for i in range(n.value):
            tid, par, rk, nm = C.c_int64(), C.c_int64(), C.c_uint32(), C.c_char_p()
            assert L.mc_db_taxon(h, i, C.byref(tid), C.byref(par), C.byref(rk), C.byref(nm)) == MC_OK
            out.append((tid.value, nm.value.decode()))
        return out
    finally:
        L.mc_destroy(h)


@pytest.mark.parametrize("case", sorted(WITNESS_CASES))
def test_model_reproduces_every_reference_line(case):
    want_lines, hitdiff, maxcand = WITNESS_CASES[case]
    rec = cli_case(case)
    z = np.load(os.path.join(GOLDEN, "toy32_expected.npz"))
    lin = z["lineages"]                                            # [targets, 21] taxon ids, 0 = none (ids stand in for indices: only equality counts)
    tgt_of = {str(nm): t for t, nm in enumerate(z["target_names"])}
    id_of_name = {}
    for tid, nm in metadata_taxa():
        id_of_name.setdefault(nm, set()).add(tid)
    hitmin = header_number(rec["lines"], "# Classification hit threshold is ")
    assert header_number(rec["lines"], "# At maximum ") == (maxcand if maxcand else 2 ** 64 - 1)
    body = [l for l in rec["lines"] if l and not l.startswith("#")]
    assert len(body) == want_lines
    factor = api.hitdiff_factor(hitdiff)
    wrong = []
    for l in body:
        cols = l.split("\t|\t")
        tophits, verdict = cols[-2], cols[-1]
        ents = [e.rsplit(":", 1) for e in tophits.split(",") if e and e != "--"]
        stride = max(maxcand if maxcand else len(ents), len(ents), 1)
        tg = np.zeros(stride, dtype=np.uint32); hi = np.zeros(stride, dtype=np.uint32)
        for j, (nm, h) in enumerate(ents):
            tg[j], hi[j] = tgt_of[nm], int(h)
        taxon, rank, _ = classify_ref.vote(lin, tg, hi, hitmin, factor, 0, classify_ref.NUM_RANKS - 1)
        if verdict == "--":
            ok = rank == classify_ref.NUM_RANKS and taxon == 0
        else:
            rname, tname = verdict.split(":", 1)
            ok = rank < classify_ref.NUM_RANKS and RANKS[rank] == rname and taxon in id_of_name.get(tname, ())
        if not ok:
            wrong.append((l, taxon, rank))
    assert not wrong, f"{len(wrong)} of {len(body)} lines differ, first: {wrong[0]}"


def test_fast_model_equals_the_plain_one():
    """vote_all_fast (what the GPU property test uses for millions of rows) against vote(), on rows that hit every branch"""
    rng = np.random.default_rng(5)
    nt = 40
    lin = rng.integers(1, 30, size=(nt, 21)).astype(np.uint32)
    lin[rng.random(lin.shape) < 0.4] = 0
    lin[:, 12:] = np.where(rng.random((nt, 9)) < 0.7, np.arange(100, 109, dtype=np.uint32)[None, :], lin[:, 12:])      # shared ancestors
    for stride in (1, 2, 4, 8):
        c = np.zeros((3000, stride), dtype=api.cand_dtype)
        c["tgt"] = rng.integers(0, nt + 3, size=c.shape)
        c["hits"] = rng.integers(0, 12, size=c.shape)
        for hm, hd, lo, hi in ((0, 1.0, 0, 20), (5, 0.5, 0, 20), (3, 0.8, 4, 16), (11, 0.0, 6, 6), (2, 0.3, 20, 20), (1, 1.0, 0, 0)):
            assert np.array_equal(classify_ref.vote_all_fast(lin, c, hm, hd, lo, hi), classify_ref.vote_all(lin, c, hm, hd, lo, hi)), (stride, hm, hd, lo, hi)


# ---- the C ABI without a device -------------------------------------------------------------------------------------------------
def test_struct_sizes_and_defaults():
    assert C.sizeof(api.McClassifyOptions) == 16 and api.assignment_dtype.itemsize == 8
    o = api.McClassifyOptions(9, 9.0, 9, 9)
    api.lib().mc_classify_options_default(C.byref(o))
    assert (o.hits_min, o.hits_diff, o.lowest_rank, o.highest_rank) == (0, 1.0, 0, 20)
    api.lib().mc_classify_options_default(None)                    # a no-op
    a = np.zeros(1, dtype=api.assignment_dtype)
    a.view("<u4")[:] = [7, 4 | (3 << 8)]                           # mc_assignment {taxon, info}
    assert (a["taxon"][0], a["rank"][0], a["voters"][0]) == (7, 4, 3)


def test_new_names_are_exported():
    L = C.CDLL(api._build.build_library())
    for n in ("mc_classify_options_default", "mc_classify_candidates", "mc_classify_tally"):
        assert hasattr(L, n) and n in api.EXPORTS


def test_python_percent_rule():
    """as the command line: a -hitdiff above 1 is a percentage, float times 0.01 in double, rounded back to float"""
    for v in (0.0, 0.5, 1.0):
        assert api.hitdiff_factor(v) == float(np.float32(v))
    for v in (80, 50, 1.5, 33.3, 100, 7):
        assert api.hitdiff_factor(v) == float(np.float32(np.float64(np.float32(v)) * 0.01))
    assert api.hitdiff_factor(80) == float(np.float32(0.8))
    o = api.classify_options(hitmin=5, hitdiff=80, lowest=4, highest=16)
    assert (o.hits_min, o.hits_diff, o.lowest_rank, o.highest_rank) == (5, np.float32(0.8), 4, 16)


def test_error_order_arguments_first_then_state():
    L = api.lib()
    h = C.c_void_p()
    assert L.mc_open_metadata(os.path.join(GOLDEN, "toy32").encode(), C.byref(h)) == MC_OK
    try:
        cands = np.zeros((4, 2), dtype=api.cand_dtype)
        out = np.zeros(4, dtype=api.assignment_dtype)
        good = api.classify_options()

        def call(ctx=h, opt=good, c=cands.ctypes.data, n=4, stride=2, flags=api.CLASSIFY_HOST, o=out.ctypes.data):
            return L.mc_classify_candidates(ctx, C.byref(opt) if opt is not None else None, c, n, stride, flags, o, None)

        assert call(ctx=None) == MC_ERR_INVALID
        assert call(opt=None) == MC_ERR_INVALID
        assert call(c=None) == MC_ERR_INVALID and call(o=None) == MC_ERR_INVALID
        assert call(stride=0) == MC_ERR_INVALID
        assert call(flags=4) == MC_ERR_INVALID
        assert call(o=cands.ctypes.data) == MC_ERR_INVALID                        # out aliases cands
        for bad in (api.McClassifyOptions(0, 1.0, -1, 20), api.McClassifyOptions(0, 1.0, 0, 21), api.McClassifyOptions(0, 1.0, 21, 21),
                    api.McClassifyOptions(0, 1.0, 5, 4), api.McClassifyOptions(0, -0.5, 0, 20), api.McClassifyOptions(0, float("inf"), 0, 20),
                    api.McClassifyOptions(0, float("nan"), 0, 20)):
            assert call(opt=bad) == MC_ERR_INVALID, (bad.hits_diff, bad.lowest_rank, bad.highest_rank)
            assert call(opt=bad, n=0) == MC_ERR_INVALID                           # arguments are looked at even when there is nothing to do
        assert L.mc_last_error(h)                                                 # (the context says what was wrong)
        # valid arguments: nothing to do is fine on any context, work needs a device -- this context has lineages but none
        assert call(n=0) == MC_OK and call(n=0, c=None, o=None) == MC_OK
        assert call() == MC_ERR_STATE and call(flags=0) == MC_ERR_STATE
        assert b"device" in L.mc_last_error(h)
        # bad arguments win over the missing device
        assert call(stride=0) == MC_ERR_INVALID
        assigned = np.zeros(22, dtype=np.uint64)
        assert L.mc_classify_tally(None, assigned.ctypes.data, None, 0, None, 0) == MC_ERR_INVALID
        assert L.mc_classify_tally(h, assigned.ctypes.data, None, 5, None, 0) == MC_ERR_INVALID
        assert L.mc_classify_tally(h, assigned.ctypes.data, None, 0, None, 0) == MC_ERR_STATE
    finally:
        L.mc_destroy(h)
