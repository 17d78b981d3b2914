"""CPU: the model of the evaluation against a ground truth (tests/evaluate_ref.py) against the reference's own summary, the taxon
table of mc_open_metadata against the model's walk, and the argument checks of mc_set_taxon_table / mc_evaluate_* that need no device.

The model is what tests/test_gpu_evaluate.py holds the device to.  Here it is itself held to the reference: the 300 mapping lines of
the golden case `ground_truth` (tests/golden/cli_expected.json.gz) carry, per read, the true taxon and the assigned one; the golden case
`precision_truth_lineage` ran on the same reads with the same classification and printed the reference's evaluation.  The model, given
those pairs and its own table of toy32's taxa, and api.Evaluation's arithmetic and formatting above its bins, must print that summary
line for line."""
import ctypes as C
import gzip
import json
import os
import re

import numpy as np
import pytest

import evaluate_ref
from metacache_amd import api

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MC_OK, MC_ERR_INVALID, MC_ERR_STATE = 0, -1, -6
NUM_RANKS = 21


def cli_case(name):
    with gzip.open(os.path.join(GOLDEN, "cli_expected.json.gz"), "rt") as f:
        return json.load(f)[name]


@pytest.fixture(scope="module")
def meta():
    """a metadata-only context of toy32 (no device) and its taxa as (id, parent, rank, name)"""
    L = api.lib()
    h = C.c_void_p()
    assert L.mc_open_metadata(os.path.join(GOLDEN, "toy32").encode(), C.byref(h)) == MC_OK
    n = C.c_uint64()
    assert L.mc_db_num_taxa(h, C.byref(n)) == MC_OK
    taxa = []
    for i in range(n.value):
        tid, par, rk, nm = C.c_int64(), C.c_int64(), C.c_uint32(), C.c_char_p()
        assert L.mc_db_taxon(h, i, C.byref(tid), C.byref(par), C.byref(rk), C.byref(nm)) == MC_OK
        taxa.append((tid.value, par.value, rk.value, nm.value.decode()))
    yield h, taxa
    L.mc_destroy(h)


def library_table(h):
    pl, pr, pc, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
    assert api.lib().mc_db_taxon_table(h, C.byref(pl), C.byref(pr), C.byref(pc), C.byref(n)) == MC_OK
    lin = api._view(pl.value, n.value * NUM_RANKS, np.dtype("<u4")).reshape(n.value, NUM_RANKS).copy()
    return lin, api._view(pr.value, n.value, np.dtype("u1")).copy(), (api._view(pc.value, n.value, np.dtype("u1")).copy() if pc.value else None)


def taxon_of_column(col, index_of_id):
    """'rank:name(taxid)' -> taxon index + 1, '--' -> 0"""
    if col == "--":
        return 0
    return index_of_id[int(re.fullmatch(r"\w+:.*\((-?\d+)\)", col).group(1))] + 1


def golden_pairs(taxa):
    """(assigned, truth) of every read of the golden case `ground_truth`, as taxon index + 1"""
    rec = cli_case("ground_truth")
    index_of_id = {t[0]: i for i, t in enumerate(taxa)}
    body = [l.split("\t|\t") for l in rec["lines"] if l and not l.startswith("#")]
    assert len(body) == 300 and all(len(c) == 3 for c in body)
    return np.array([taxon_of_column(c[2], index_of_id) for c in body], dtype=np.uint32), np.array([taxon_of_column(c[1], index_of_id) for c in body], dtype=np.uint32)


def summary_of(rec):
    lines = rec["lines"]
    first = next(i for i, l in enumerate(lines) if l.startswith("# unclassified:"))
    return [l for l in lines[first:] if l]


def test_model_and_summary_reproduce_the_reference_evaluation(meta):
    _, taxa = meta
    lin, rank, covered = evaluate_ref.taxon_table(taxa)
    assigned, truth = golden_pairs(taxa)
    _, want = evaluate_ref.evaluate(lin, rank, covered, assigned, truth)
    ev = api.Evaluation(want["assigned"], want["known"], want["correct"], want["wrong"], want["coverage"], want["reads"], want["out_of_table"])
    golden = summary_of(cli_case("precision_truth_lineage"))
    assert len(golden) == 1 + 5 * 12 + 1 and golden[-1].startswith("#   root")
    assert ev.summary_lines("# ") == golden
    # the figures themselves, as they were worked out by hand from the same lines
    assert ev.unknown() == 67 and ev.known(0) == ev.known(3) == 200 and ev.known(4) == ev.known(20) == 233 and ev.total() == 300
    assert [ev.correct(r) for r in ev.SUMMARY_RANKS] == [3, 3, 18, 18, 18, 24, 49, 136, 136, 136, 136]
    assert f"{100 * ev.precision(0):g}" == "1.47059" and f"{100 * ev.precision(20):g}" == "58.6207"
    assert f"{100 * ev.sensitivity(0):g}" == "1.5" and f"{100 * ev.sensitivity(20):g}" == "58.3691"


def test_fast_model_is_the_plain_one():
    """evaluate (every distinct pair once, weighted) against evaluate_plain (read by read) on a synthetic table: the form that models the
    GPU tests' long lists is the rule itself"""
    lin, rank, covered = evaluate_ref.taxon_table(evaluate_ref.synthetic_taxa(np.random.default_rng(7)))
    a, t = evaluate_ref.random_pairs(np.random.default_rng(3), 400, len(lin), lin)
    v1, b1 = evaluate_ref.evaluate_plain(lin, rank, covered, a, t, True)
    v2, b2 = evaluate_ref.evaluate(lin, rank, covered, a, t, True)
    assert np.array_equal(v1, v2) and all(np.array_equal(b1[k], b2[k]) for k in b1)
    assert b1["out_of_table"] > 0 and b1["wrong"].sum() > 0 and (b1["coverage"].sum(axis=0) > 0).all()      # (every kind of counter is in play)


def test_summary_of_nothing_classified():
    ev = api.Evaluation([0] * 21 + [5], [0] * 22, [0] * 22, [0] * 22)
    assert ev.summary_lines() == ["None of the input sequences could be classified."]


def test_taxon_table_of_the_metadata_equals_the_models_walk(meta):
    h, taxa = meta
    lin, rank, covered = library_table(h)
    wlin, wrank, wcovered = evaluate_ref.taxon_table(taxa)
    for x in range(len(taxa)):
        assert np.array_equal(lin[x], wlin[x]), f"row of taxon {x} ({taxa[x]})"
    assert np.array_equal(rank, wrank) and covered is not None and np.array_equal(covered, wcovered)
    assert np.array_equal(rank, evaluate_ref.derived_rank(lin))                      # what rank == NULL would derive
    # the targets' rows are the rows of mc_db_lineages
    pl, nt = C.c_void_p(), C.c_uint64()
    assert api.lib().mc_db_lineages(h, C.byref(pl), C.byref(nt)) == MC_OK
    tlin = api._view(pl.value, nt.value * NUM_RANKS, np.dtype("<u4")).reshape(nt.value, NUM_RANKS)
    index_of_id = {t[0]: i for i, t in enumerate(taxa)}
    for t in range(nt.value):
        assert np.array_equal(lin[index_of_id[-t - 1]], tlin[t]), f"target {t}"
    # the counts of toy32, from an independent parent walk
    targets = [i for i, t in enumerate(taxa) if t[0] < 0]
    assert len(taxa) == 106 and len(targets) == nt.value == 24
    assert int((covered != 0).sum()) == 63 and int((covered == 0).sum()) == 43 and int((rank == NUM_RANKS).sum()) == 19
    by_id = {t[0]: i for i, t in enumerate(taxa)}
    for i in targets:                                                                # no target with two ancestors of one rank
        ranks = [taxa[j][2] for j in evaluate_ref.parent_chain(taxa, by_id, i) if taxa[j][2] < NUM_RANKS]
        assert len(ranks) == len(set(ranks))


def test_arguments_are_checked_before_the_state(meta):
    """every MC_ERR_INVALID case on a context that has a table but no device: what is left over is MC_ERR_STATE"""
    h, taxa = meta
    L = api.lib()
    n = 8
    assigned = np.zeros(n, dtype=api.assignment_dtype)
    truth = np.zeros(n, dtype=np.uint32)
    verdicts = np.zeros(n, dtype=api.verdict_dtype)
    A, T, V = assigned.ctypes.data, truth.ctypes.data, verdicts.ctypes.data
    HOST, TALLY, COV = api.EVALUATE_HOST, api.EVALUATE_TALLY, api.EVALUATE_COVERAGE
    ev = L.mc_evaluate_assignments
    assert ev(None, A, T, n, HOST | TALLY, V, None) == MC_ERR_INVALID                # no context
    assert ev(h, None, T, n, HOST | TALLY, V, None) == MC_ERR_INVALID                # null arrays
    assert ev(h, A, None, n, HOST | TALLY, V, None) == MC_ERR_INVALID
    assert ev(h, A, T, n, HOST, None, None) == MC_ERR_INVALID                        # neither verdicts nor TALLY
    assert ev(h, A, T, n, HOST | COV, V, None) == MC_ERR_INVALID                     # COVERAGE without TALLY
    assert ev(h, A, T, n, HOST | TALLY | 8, V, None) == MC_ERR_INVALID               # unknown flag
    assert ev(h, A + 4, T, n - 1, TALLY, V, None) == MC_ERR_INVALID                  # misaligned "device" arrays
    assert ev(h, A, T + 2, n - 1, TALLY, V, None) == MC_ERR_INVALID
    assert ev(h, A, T, n - 1, TALLY, V + 1, None) == MC_ERR_INVALID
    assert ev(h, A, T, n, HOST | TALLY, A + 8, None) == MC_ERR_INVALID               # verdicts overlapping an input
    assert ev(h, A, T, n, HOST | TALLY, T, None) == MC_ERR_INVALID
    assert b"overlaps" in L.mc_last_error(h)
    assert ev(h, None, None, 0, HOST | TALLY, None, None) == MC_OK                   # nothing to do
    assert ev(h, A, T, n, HOST | TALLY, V, None) == MC_ERR_STATE                     # a table, but no device
    assert b"no device" in L.mc_last_error(h)
    e = api.McEvaluation()
    assert L.mc_evaluate_tally(None, C.byref(e), 0) == MC_ERR_INVALID
    assert L.mc_evaluate_tally(h, None, 0) == MC_ERR_INVALID
    assert L.mc_evaluate_tally(h, C.byref(e), 0) == MC_ERR_STATE


def test_set_taxon_table_checks_and_keeps_what_it_is_given(meta):
    _, taxa = meta
    L = api.lib()
    h = C.c_void_p()
    assert L.mc_open_metadata(os.path.join(GOLDEN, "toy32").encode(), C.byref(h)) == MC_OK      # a context of its own: the table is replaced
    try:
        lin = np.zeros((5, NUM_RANKS), dtype=np.uint32)
        lin[0, 20] = 1
        lin[1, 4], lin[1, 20] = 2, 1
        lin[2, 20] = 1                                                                # taxon 3 has no rank of its own
        lin[3, 0], lin[3, 4], lin[3, 20] = 4, 2, 1
        lin[4, 0] = 5
        covered = np.array([1, 1, 0, 1, 0], dtype=np.uint8)
        st = L.mc_set_taxon_table
        assert st(None, lin.ctypes.data, None, None, 5) == MC_ERR_INVALID
        assert st(h, None, None, None, 5) == MC_ERR_INVALID
        assert st(h, lin.ctypes.data, None, None, 2 ** 32 - 1) == MC_ERR_INVALID
        bad = lin.copy(); bad[4, 7] = 6
        assert st(h, bad.ctypes.data, None, None, 5) == MC_ERR_INVALID
        assert b"beyond the table" in L.mc_last_error(h)
        assert library_table(h)[0].shape == (len(taxa), NUM_RANKS)                    # a refused table changes nothing
        assert st(h, lin.ctypes.data, None, None, 5) == MC_OK                         # no rank: derived; no covered: none
        got = library_table(h)
        assert np.array_equal(got[0], lin) and got[1].tolist() == [20, 4, 21, 0, 0] and got[2] is None
        n = 4
        assigned = np.zeros(n, dtype=api.assignment_dtype); truth = np.zeros(n, dtype=np.uint32); verdicts = np.zeros(n, dtype=api.verdict_dtype)
        flags = api.EVALUATE_HOST | api.EVALUATE_TALLY | api.EVALUATE_COVERAGE
        assert L.mc_evaluate_assignments(h, assigned.ctypes.data, truth.ctypes.data, n, flags, verdicts.ctypes.data, None) == MC_ERR_STATE
        assert b"covered" in L.mc_last_error(h)                                       # (before the missing device is looked at)
        rank = np.array([20, 4, 21, 0, 200], dtype=np.uint8)                          # beyond MC_NUM_RANKS: read as none
        assert st(h, lin.ctypes.data, rank.ctypes.data, covered.ctypes.data, 5) == MC_OK
        got = library_table(h)
        assert got[1].tolist() == [20, 4, 21, 0, 21] and np.array_equal(got[2], covered)
        assert st(h, None, None, None, 0) == MC_OK and library_table(h)[0].shape == (0, NUM_RANKS)
    finally:
        L.mc_destroy(h)
