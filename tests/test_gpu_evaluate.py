"""GPU: mc_evaluate_assignments / mc_evaluate_tally (taxon_evaluate_kernel) -- how good a classification was, given the truth.

  * against the model (tests/evaluate_ref.py, itself held to the reference's summary by test_evaluate_witness_cpu.py): verdict by verdict
    and counter by counter, on toy32's own taxon table and on a synthetic one set with mc_set_taxon_table (about 3 000 taxa: random
    depth, ranks skipped, taxa without a rank, taxa no target covers, and one chain that has a taxon of every rank); the sizes around a
    wave and a block, a size that makes the capped grid stride, every class of pair by itself, one pair for all reads and all pairs
    distinct, two streams tallying at once, reset, the host form across three staged pieces, the coverage counters with and without
    a covered array, a table whose rank array disagrees with its slots;
  * against the reference: query, vote and evaluation enqueued on one stream without a synchronisation in between, on the reads of
    tests/golden/cli_truth.fa with the truths the reference read from their headers; the tallies must print the reference's summary."""
import gzip
import json
import os
import re

import numpy as np
import pytest

import evaluate_ref
from metacache_amd import api

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NUM_RANKS = 21
GRID_CAP, BLOCK = 2048, 256                    # taxon_evaluate_kernel's launch: beyond GRID_CAP * BLOCK reads the blocks stride


@pytest.fixture(scope="module")
def synth():
    rng = np.random.default_rng(7)
    taxa = evaluate_ref.synthetic_taxa(rng)
    lin, rank, covered = evaluate_ref.taxon_table(taxa)
    assert 2900 < len(taxa) < 3100 and (rank == NUM_RANKS).sum() > 100 and 200 < (covered == 0).sum() and (covered != 0).sum() > 600
    assert (np.count_nonzero(lin, axis=1) == NUM_RANKS).any() and (np.count_nonzero(lin, axis=1) < 5).any()
    return taxa, lin, rank, covered


@pytest.fixture(scope="module")
def db():
    d = api.Database.open(os.path.join(GOLDEN, "toy32"), max_candidates=2)
    yield d
    d.close()


def on_device(torch, assigned, truth):
    dev = torch.device("cuda", 0)
    a = np.zeros(len(assigned), dtype=api.assignment_dtype)
    a["taxon"] = assigned
    a["rank"] = 77                                                            # (what a producer wrote there is not read)
    da = torch.from_numpy(a.view(np.int32).reshape(len(a), 2).copy()).to(dev)
    dt = torch.from_numpy(np.asarray(truth, dtype=np.uint32).view(np.int32).copy()).to(dev)
    return da, dt, torch.empty(max(len(a), 1), dtype=torch.int32, device=dev)


def run_device(db, assigned, truth, coverage=False, tally=True, want_verdicts=True):
    import torch
    n = len(truth)
    da, dt, dv = on_device(torch, assigned, truth)
    torch.cuda.synchronize()
    db.evaluate_device(da.data_ptr(), dt.data_ptr(), n, tally=tally, coverage=coverage, verdicts_ptr=dv.data_ptr() if want_verdicts else 0)
    db.synchronize()
    return dv[:n].cpu().numpy().view(api.verdict_dtype).reshape(n)


def as_triples(v):
    assert not v["reserved"].any()
    return np.stack([v["known"], v["correct"], v["flags"]], axis=1)


def check(db, table, assigned, truth, coverage, what):
    lin, rank, covered = table
    got = run_device(db, assigned, truth, coverage=coverage)
    want_v, want = evaluate_ref.evaluate(lin, rank, covered, assigned, truth, coverage)
    bad = np.flatnonzero((as_triples(got) != want_v).any(axis=1))
    assert bad.size == 0, (what, bad.size, int(bad[0]), int(assigned[bad[0]]), int(truth[bad[0]]), got[bad[0]], want_v[bad[0]])
    ev = db.evaluation(reset=True)
    assert evaluate_ref.same_counters(ev, want) == [], (what, evaluate_ref.same_counters(ev, want))
    return want


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_sizes_around_a_wave_and_a_block(db, synth, n):
    _, lin, rank, covered = synth
    db.set_taxon_table(lin, rank, covered)
    a, t = evaluate_ref.random_pairs(np.random.default_rng(100 + n), n, len(lin), lin)
    if n == 0:                                                                # nothing is done, nothing is counted, null arrays are fine
        db.evaluate_device(0, 0, 0, tally=True, coverage=True)
        assert db.evaluation().total() == 0 and db.evaluation().reads == 0
        return
    want = check(db, (lin, rank, covered), a, t, True, f"n = {n}")
    assert want["reads"] == n


def test_blocks_stride_over_more_reads_than_the_grid_holds(db, synth):
    _, lin, rank, covered = synth
    db.set_taxon_table(lin, rank, covered)
    rng = np.random.default_rng(11)
    n = GRID_CAP * BLOCK + 300
    pa, pt = evaluate_ref.random_pairs(rng, 2500, len(lin), lin)                           # the reads draw from 2 500 pairs (the model judges each once)
    pick = rng.integers(0, len(pa), n)
    want = check(db, (lin, rank, covered), pa[pick], pt[pick], True, "strided grid")
    assert want["out_of_table"] > 0 and want["wrong"].sum() > 0 and want["coverage"][:, 1].sum() > 0


def pairs_by_class(taxa, lin, rank):
    """name -> (assigned, truth) lists, every class of pair the rule tells apart"""
    n = len(taxa)
    ranked = [i + 1 for i in range(n) if rank[i] < NUM_RANKS]
    unranked = [i + 1 for i in range(n) if rank[i] == NUM_RANKS]
    deep = [x for x in ranked if np.count_nonzero(lin[x - 1]) >= 4][:200]
    out = {
        "unclassified": ([0] * len(deep), deep),
        "truth unknown": (deep, [0] * len(deep)),
        "neither": ([0] * 70, [0] * 70),
        "the same taxon": (ranked[:300], ranked[:300]),
        "assigned is an ancestor": ([int(lin[x - 1][np.nonzero(lin[x - 1])[0][-2]]) for x in deep], deep),
        "truth is an ancestor": (deep, [int(lin[x - 1][np.nonzero(lin[x - 1])[0][-2]]) for x in deep]),
        "truth without a rank": (deep[:len(unranked)], unranked[:len(deep)]),
        "assigned without a rank": (unranked[:len(deep)], deep[:len(unranked)]),
        "beyond the table": ([n + 1, 0xFFFFFFFF, 5, n + 1, n], [7, n + 2, n + 1, n + 9, n]),
    }
    # siblings under every rank: the two targets under the chain's taxon of rank r (ids -1 .. -40 in evaluate_ref.synthetic_taxa's order)
    index_of_id = {t[0]: i for i, t in enumerate(taxa)}
    sib_a, sib_t = [], []
    for k in range(20):
        sib_a.append(index_of_id[-(2 * k + 1)] + 1); sib_t.append(index_of_id[-(2 * k + 2)] + 1)
    out["siblings under every rank"] = (sib_a, sib_t)
    return out


def test_every_class_of_pair_by_itself(db, synth):
    taxa, lin, rank, covered = synth
    db.set_taxon_table(lin, rank, covered)
    classes = pairs_by_class(taxa, lin, rank)
    for name, (a, t) in classes.items():
        a, t = np.array(a, dtype=np.uint32), np.array(t, dtype=np.uint32)
        assert len(a) == len(t) > 0, name
        want = check(db, (lin, rank, covered), a, t, True, name)
        if name == "siblings under every rank":                               # the LCA of pair k is the chain's taxon of rank 20 - k
            v, _ = evaluate_ref.evaluate(lin, rank, covered, a, t)
            assert v[:, 1].tolist() == list(range(20, 0, -1)) and v[:, 2].all()
            assert want["wrong"][:20].tolist() == [1] * 20
        if name == "beyond the table":
            assert want["out_of_table"] == 6


def test_one_pair_for_all_reads_and_all_pairs_distinct(db, synth):
    taxa, lin, rank, covered = synth
    db.set_taxon_table(lin, rank, covered)
    n = 3000
    index_of_id = {t[0]: i for i, t in enumerate(taxa)}
    a, t = index_of_id[-1] + 1, index_of_id[-40] + 1                          # a wrong call under the root: every lane on the same bins
    want = check(db, (lin, rank, covered), np.full(n, a, dtype=np.uint32), np.full(n, t, dtype=np.uint32), True, "one pair")
    assert want["wrong"][19] == n and want["coverage"].max() == n
    rng = np.random.default_rng(5)
    n = len(lin) - 99                                                         # 2 900: no taxon twice on either side
    a = rng.permutation(len(lin))[:n].astype(np.uint32) + 1
    t = rng.permutation(len(lin))[:n].astype(np.uint32) + 1
    assert len(set(a.tolist())) == len(set(t.tolist())) == n
    check(db, (lin, rank, covered), a, t, True, "distinct pairs")


def test_two_streams_tally_at_the_same_time_and_reset_clears(db, synth):
    import torch
    _, lin, rank, covered = synth
    db.set_taxon_table(lin, rank, covered)
    rng = np.random.default_rng(21)
    n = 200_000
    pa, pt = evaluate_ref.random_pairs(rng, 2000, len(lin), lin)
    pick = rng.integers(0, len(pa), 2 * n)
    a, t = pa[pick], pt[pick]
    da, dt, _ = on_device(torch, a, t)
    streams = [torch.cuda.Stream(device=torch.device("cuda", 0)) for _ in range(2)]
    torch.cuda.synchronize()
    assert db.evaluation(reset=True) is not None and db.evaluation().reads == 0
    for _ in range(3):
        for j, st in enumerate(streams):
            db.evaluate_device(da[j * n:].data_ptr(), dt[j * n:].data_ptr(), n, tally=True, coverage=True, stream=st.cuda_stream)
    for st in streams:
        st.synchronize()
    _, want = evaluate_ref.evaluate(lin, rank, covered, a, t, True)
    want = {k: v * (np.uint64(3) if isinstance(v, np.ndarray) else 3) for k, v in want.items()}
    ev = db.evaluation(reset=True)
    assert evaluate_ref.same_counters(ev, want) == []
    after = db.evaluation()
    assert after.reads == 0 and not after.bins.any() and not after.confusion.any()
    # verdicts alone leave the counters as they are
    run_device(db, a[:1000], t[:1000], tally=False)
    assert db.evaluation().reads == 0


def test_host_form_across_three_pieces(db, synth):
    _, lin, rank, covered = synth
    db.set_taxon_table(lin, rank, covered)
    db.set_tuning("evaluate_stage_rows", 400)
    try:
        a, t = evaluate_ref.random_pairs(np.random.default_rng(31), 1000, len(lin), lin)
        assigned = np.zeros(1000, dtype=api.assignment_dtype)
        assigned["taxon"] = a
        db.evaluation(reset=True)
        db.timing(True); db.timing_reset()
        got = db.evaluate(assigned, t, coverage=True)
        ms, launches = db.timing_get("taxon_evaluate")
        db.timing(False)
        assert launches == 3 and ms > 0                                       # 400 + 400 + 200
        want_v, want = evaluate_ref.evaluate(lin, rank, covered, a, t, True)
        assert np.array_equal(as_triples(got), want_v)
        assert evaluate_ref.same_counters(db.evaluation(reset=True), want) == []
    finally:
        db.set_tuning("evaluate_stage_rows", 0)


def test_coverage_needs_a_covered_array_and_ranks_come_from_the_table(db, synth):
    _, lin, rank, covered = synth
    a, t = evaluate_ref.random_pairs(np.random.default_rng(41), 2000, len(lin), lin)
    db.set_taxon_table(lin, rank, None)                                       # no covered array: the counters of -taxon-coverage cannot be had
    with pytest.raises(api.McError, match="covered"):
        run_device(db, a, t, coverage=True)
    check(db, (lin, rank, covered), a, t, False, "no covered array")
    db.set_taxon_table(lin, None, covered)                                    # no rank array: derived from the rows -- the same table
    check(db, (lin, rank, covered), a, t, True, "derived ranks")
    odd = rank.copy()                                                         # a rank array that disagrees with the slots: the ARRAY decides
    rng = np.random.default_rng(42)
    odd[rng.integers(0, len(odd), 150)] = rng.integers(0, NUM_RANKS + 1, 150).astype(np.uint8)
    db.set_taxon_table(lin, odd, covered)
    check(db, (lin, odd, covered), a, t, True, "ranks that disagree with the slots")
    # a new table starts the tallies from zero
    run_device(db, a, t)
    assert db.evaluation().reads == len(a)
    db.set_taxon_table(lin, rank, covered)
    assert db.evaluation().reads == 0


# ---- the chain, against the reference ------------------------------------------------------------------------------------------------
def cli_case(name):
    with gzip.open(os.path.join(GOLDEN, "cli_expected.json.gz"), "rt") as f:
        return json.load(f)[name]


def read_fasta(path):
    recs = []
    with open(path, "rb") as f:
        for line in f.read().split(b"\n"):
            if line.startswith(b">"):
                recs.append([line[1:].split()[0].decode(), b""])
            elif line.strip():
                recs[-1][1] += line.strip()
    return [(h, s) for h, s in recs if s]


def test_query_vote_and_evaluation_on_one_stream_print_the_reference_summary():
    import torch
    recs = read_fasta(os.path.join(GOLDEN, "cli_truth.fa"))
    reads = [s for _, s in recs]
    truth_rec = cli_case("ground_truth")
    body = [l.split("\t|\t") for l in truth_rec["lines"] if l and not l.startswith("#")]
    assert [c[0] for c in body] == [h for h, _ in recs]
    golden = cli_case("precision_truth_lineage")["lines"]
    first = next(i for i, l in enumerate(golden) if l.startswith("# unclassified:"))
    summary = [l for l in golden[first:] if l]
    dev = torch.device("cuda", 0)
    d = api.Database.open(os.path.join(GOLDEN, "toy32"), max_candidates=2)
    try:
        index_of_id = {t[0]: i for i, t in enumerate(d.taxa())}
        truth = np.array([0 if c[1] == "--" else index_of_id[int(re.fullmatch(r"\w+:.*\((-?\d+)\)", c[1]).group(1))] + 1 for c in body], dtype=np.uint32)
        n = len(reads)
        pad = [len(r) + (-len(r)) % 4 for r in reads]
        offs = np.concatenate([[0], np.cumsum(pad)]).astype(np.int64)
        buf = np.zeros(int(offs[-1]) + 16, dtype=np.uint8)
        for r, o in zip(reads, offs[:-1]):
            buf[o:o + len(r)] = np.frombuffer(r, dtype=np.uint8)
        qinfo = np.zeros((n, 4), dtype=np.uint32)
        qinfo[:, 0] = offs[:-1]; qinfo[:, 1] = [len(r) for r in reads]; qinfo[:, 2] = offs[:-1]
        mw = np.array([d.max_windows_in_range(len(r)) for r in reads], dtype=np.int32)
        seq, qi, dmw = torch.from_numpy(buf).to(dev), torch.from_numpy(qinfo.view(np.int32)).to(dev), torch.from_numpy(mw).to(dev)
        dt = torch.from_numpy(truth.view(np.int32)).to(dev)
        out = torch.empty((n, 2), dtype=torch.int32, device=dev)
        verdicts = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        # the reference's defaults (the golden case's header): hit threshold 5, two candidates, ranks sequence .. domain
        r = d.query_device(seq.data_ptr(), qi.data_ptr(), n, int(offs[-1]), max_win_ptr=dmw.data_ptr())
        d.classify_device(r.cands, n, 2, out_ptr=out.data_ptr(), hitmin=5, hitdiff=1.0, lowest=0, highest=19)
        d.evaluate_device(out.data_ptr(), dt.data_ptr(), n, tally=True, verdicts_ptr=verdicts.data_ptr())
        d.synchronize()
        ev = d.evaluation()
        assert ev.reads == n == 300 and ev.out_of_table == 0
        assert ev.summary_lines("# ") == summary
        # ... and the verdicts say what the counters say
        v = verdicts.cpu().numpy().view(api.verdict_dtype)
        assert int((v["known"] == NUM_RANKS).sum()) == ev.unknown() == 67 and int((v["flags"] & 1).sum()) == ev.wrong()
        # toy32's own table (what mc_open_database made of the .meta file), any pairs, with the coverage counters
        lin, rank, covered = d.taxon_table()
        a, t = evaluate_ref.random_pairs(np.random.default_rng(51), 5000, len(lin), lin)
        d.evaluation(reset=True)
        want = check(d, (lin, rank, covered), a, t, True, "toy32's table")
        assert want["coverage"][:, 1].sum() > 0 and want["coverage"][:, 0].sum() > 0
    finally:
        d.close()
