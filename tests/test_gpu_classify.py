"""GPU: mc_classify_candidates / mc_classify_tally (taxon_vote_kernel) -- one taxon per read from its top candidates.

  * against the reference: the reads of tests/golden/cli_reads.fa / cli_pairs.fq through Database.classify with each golden case's own
    options, every read compared with the line the reference CLI wrote for it (tests/golden/cli_expected.json.gz); the tallies against
    the reference's summary and its -abundances table;
  * against the numpy model (tests/classify_ref.py, itself held to the reference by test_classify_witness_cpu.py): random lineage
    tables and 10^6 random candidate rows per stride, device form and host form, tallies included;
  * composition: mc_query_device and mc_classify_candidates enqueued on one stream without a synchronisation in between, on both
    pipes, against the slot path; two streams tallying at the same time; reset."""
import gzip
import json
import os
import re

import numpy as np
import pytest

import classify_ref
from cpuref import RANKS
from metacache_amd import api

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NUM_RANKS = 21


# ---- the golden cases ---------------------------------------------------------------------------------------------------------
def cli_case(name):
    with gzip.open(os.path.join(GOLDEN, "cli_expected.json.gz"), "rt") as f:
        return json.load(f)[name]


def read_fasta(path):
    """[(first word of the header, sequence)]; sequences may span lines, blank lines are skipped"""
    recs = []
    with open(path, "rb") as f:
        for line in f.read().split(b"\n"):
            if line.startswith(b">"):
                recs.append([line[1:].split()[0].decode(), b""])
            elif line.strip():
                recs[-1][1] += line.strip()
    return [(h, s) for h, s in recs]


def read_fastq(path):
    with open(path, "rb") as f:
        lines = f.read().split(b"\n")
    return [(lines[i][1:].split()[0].decode(), lines[i + 1].strip()) for i in range(0, len(lines) - 3, 4)]


def option_value(args, name, default):
    return args[args.index(name) + 1] if name in args else default


def case_setup(rec):
    """the options a golden case ran with, from its argument list and from what the reference printed about itself"""
    lines, args = rec["lines"], rec["args"]
    head = "\n".join(l for l in lines if l.startswith("#"))
    lowest, highest = re.search(r"constrained to ranks from '(\w+)' to '(\w+)'", head).groups()
    hitmin = int(re.search(r"Classification hit threshold is (\d+)", head).group(1))
    maxcand = int(option_value(args, "-maxcand", re.search(r"At maximum (\d+) classification candidates", head).group(1)))
    layout = next(l for l in lines if l.startswith("# TABLE_LAYOUT: "))[len("# TABLE_LAYOUT: "):].split("\t|\t")
    return dict(hitmin=hitmin, hitdiff=float(option_value(args, "-hitdiff", 1.0)), lowest=RANKS.index(lowest), highest=RANKS.index(highest),
                insert_max=int(option_value(args, "-insertsize", 0)), maxcand=maxcand, pairs="-pairseq" in args,
                header_col=layout.index("query_header"), ids_only="-taxids-only" in args)


def verdict_matches(verdict, ids_only, a, taxa):
    """does assignment a (taxon, rank, voters) say what the reference's last column says?"""
    taxon, rank = int(a["taxon"]), int(a["rank"])
    if ids_only:                                               # the taxon's id alone, 0 = unclassified
        return (taxon == 0 and rank == NUM_RANKS) if verdict == "0" else (taxon > 0 and taxa[taxon - 1][0] == int(verdict))
    first = verdict.split(",")[0]                              # (-lineage: the lowest match comes first)
    if first == "--":
        return taxon == 0 and rank == NUM_RANKS
    rname, tname = first.split(":", 1)
    m = re.fullmatch(r"(.*)\((-?\d+)\)", tname)                # -taxids: name(id)
    if m and taxon > 0 and taxa[taxon - 1][0] != int(m.group(2)):
        return False
    if m:
        tname = m.group(1)
    return taxon > 0 and rank < NUM_RANKS and RANKS[rank] == rname and taxa[taxon - 1][3] == tname and taxa[taxon - 1][2] == rank


def case_reads(rec, pairs):
    recs = []
    for fn in rec["files"]:
        recs += read_fastq(os.path.join(GOLDEN, fn)) if fn.endswith(".fq") else read_fasta(os.path.join(GOLDEN, fn))
    if pairs:
        return [recs[i][0] for i in range(0, len(recs), 2)], [recs[i][1] for i in range(0, len(recs), 2)], [recs[i + 1][1] for i in range(0, len(recs), 2)]
    recs = [(h, s) for h, s in recs if s]                      # a record without characters is no query
    return [h for h, _ in recs], [s for _, s in recs], None


def classify_case(name, tally=False):
    rec = cli_case(name)
    o = case_setup(rec)
    headers, reads, mates = case_reads(rec, o["pairs"])
    db = api.Database.open(os.path.join(GOLDEN, "toy32"), max_candidates=o["maxcand"])
    try:
        got = db.classify(reads, mates, hitmin=o["hitmin"], hitdiff=o["hitdiff"], lowest=o["lowest"], highest=o["highest"],
                          insert_max=o["insert_max"], tally=tally)
        return rec, o, headers, got, db.taxa(), (db.tally() if tally else None)
    finally:
        db.close()


@pytest.mark.parametrize("name", ["default", "genus_family_idsonly", "hitdiff_percent", "mapped_only_vote", "everything_species", "pairseq_insert"])
def test_every_read_as_the_reference_classified_it(name):
    rec, o, headers, got, taxa, _ = classify_case(name)
    compare_with_reference_lines(name, rec, o, headers, got, taxa)


def compare_with_reference_lines(name, rec, o, headers, got, taxa):
    body = [l.split("\t|\t") for l in rec["lines"] if l and not l.startswith("#")]
    verdict = {c[o["header_col"]]: c[-1] for c in body}
    assert len(verdict) == len(body) and set(verdict) <= set(headers) and len(set(headers)) == len(headers)
    if "-mapped-only" not in rec["args"]:
        assert len(body) == len(headers)                                     # one line per read: none is left out
    wrong = []
    for h, a in zip(headers, got):
        if h in verdict:
            ok = verdict_matches(verdict[h], o["ids_only"], a, taxa)
        else:                                                                # -mapped-only left it out: the device must leave it unclassified
            ok = int(a["taxon"]) == 0 and int(a["rank"]) == NUM_RANKS and int(a["voters"]) == 0
        if not ok:
            wrong.append((h, verdict.get(h), tuple(int(a[f]) for f in ("taxon", "rank", "voters"))))
    assert not wrong, f"{name}: {len(wrong)} of {len(headers)} reads differ, first: {wrong[:3]}"


def test_tallies_equal_the_reference_summary_and_abundances():
    rec, o, headers, got, taxa, (assigned, counts) = classify_case("default", tally=True)
    compare_with_reference_tallies(rec, headers, got, taxa, assigned, counts)


def compare_with_reference_tallies(rec, headers, got, taxa, assigned, counts):
    head = [l for l in rec["lines"] if l.startswith("#")]
    unclassified = int(re.search(r"\((\d+)\)", next(l for l in head if l.startswith("# unclassified:"))).group(1))
    assert unclassified == 112 and int(assigned[NUM_RANKS]) == unclassified
    assert int(assigned.sum()) == len(headers) == 399
    cumulative = np.cumsum(assigned[:NUM_RANKS])
    seen = {}
    for l in head:
        m = re.fullmatch(r"#\s+(\w+)\s+[\d.e+-]+% \((\d+)\)", l)
        if m and m.group(1) in RANKS:
            seen[m.group(1)] = int(m.group(2))
            assert int(cumulative[RANKS.index(m.group(1))]) == int(m.group(2)), l
    assert seen["species"] == 211 and seen["class"] == 257 and seen["phylum"] == 287
    # per taxon: the "number of reads" column of the reference's -abundances table for the same reads and options
    ab = cli_case("abundances")["lines"]
    rows = ab[ab.index("# rank:name\t|\ttaxid\t|\tnumber of reads\t|\tabundance") + 1:]
    rows = [r.split("\t|\t") for r in rows[:next(i for i, r in enumerate(rows) if r.startswith("#"))]]
    index_of = {(RANKS[t[2]], t[3]): i for i, t in enumerate(taxa) if t[2] < NUM_RANKS}
    want = np.zeros(len(counts), dtype=np.uint64)
    for r in rows:
        if r[0] == "unclassified":
            assert int(r[-2]) == int(assigned[NUM_RANKS])
            continue
        rname, tname = r[0].split(":", 1)
        want[index_of[(rname, tname)] + 1] = int(r[2])
    assert np.array_equal(counts, want)
    assert np.array_equal(counts, np.bincount(got["taxon"][got["taxon"] > 0], minlength=len(counts)).astype(np.uint64))


# ---- random tables and rows against the model -------------------------------------------------------------------------------------
def random_lineages(rng, nt):
    """[nt, 21] taxon index + 1: slot 0 the target's own taxon, above it groups that shrink in number rank by rank (shared ancestors at
    every depth), holes everywhere, some targets without a sequence-level taxon, some without anything"""
    lin = np.zeros((nt, NUM_RANKS), dtype=np.uint32)
    lin[:, 0] = np.arange(1, nt + 1)
    nxt = nt + 1
    for r in range(1, NUM_RANKS):
        groups = max(1, int(nt / 1.6 ** r))
        lin[:, r] = nxt + (np.arange(nt, dtype=np.int64) * groups) // nt
        nxt += groups
    lin[:, 1:][rng.random((nt, NUM_RANKS - 1)) < 0.45] = 0
    lin[rng.random(nt) < 0.05, 0] = 0
    lin[rng.random(nt) < 0.02] = 0
    return lin


def random_rows(rng, n, stride, nt):
    """candidate rows: neighbours in target order (common ancestors at every depth), ties, hit counts around the thresholds of
    the option sets below, terminators with leftovers behind them, empty rows, targets outside the table"""
    c = np.zeros((n, stride), dtype=api.cand_dtype)
    base = rng.integers(0, nt, size=n)
    reach = 2 ** rng.integers(0, 13, size=(n, stride))
    tgt = (base[:, None] + rng.integers(0, reach)) % nt
    tgt[:, 0] = base
    tgt = np.where(rng.random((n, stride)) < 0.02, rng.choice(np.array([nt, nt + 1, 2 ** 31, 2 ** 32 - 1]), size=(n, stride)), tgt)
    top = rng.integers(1, 61, size=n)
    kind = rng.integers(0, 4, size=(n, stride))
    near_half = np.maximum(top[:, None] - 5, 0) // 2 + rng.integers(-1, 2, size=(n, stride))       # around (top - 5) * 0.5
    hits = np.select([kind == 0, kind == 1, kind == 2], [np.broadcast_to(top[:, None], (n, stride)), top[:, None] - rng.integers(0, 4, size=(n, stride)), near_half],
                     rng.integers(0, 64, size=(n, stride)))
    hits = np.maximum(hits, 0)
    hits[rng.random((n, stride)) < 0.12] = 0                                                        # the list ends here, whatever follows
    hits[:, 0] = np.where(rng.random(n) < 0.03, 0, top)
    c["tgt"] = tgt.astype(np.uint32); c["hits"] = hits.astype(np.uint32)
    c["beg"] = rng.integers(0, 1000, size=(n, stride)); c["end"] = c["beg"] + 3
    return c


def device_vote(db, torch, dcands, n, stride, out, stream=0, **opt):
    db.classify_device(dcands.data_ptr(), n, stride, out_ptr=out.data_ptr(), stream=stream, **opt)


def as_triples(a):
    return np.stack([a["taxon"].astype(np.int64), a["rank"].astype(np.int64), a["voters"].astype(np.int64)], axis=1)


FULL_SETS = [dict(hitmin=0, hitdiff=1.0, lowest=0, highest=20), dict(hitmin=5, hitdiff=0.5, lowest=0, highest=19),
             dict(hitmin=5, hitdiff=80, lowest=4, highest=16), dict(hitmin=40, hitdiff=0.25, lowest=6, highest=10),
             dict(hitmin=7, hitdiff=0.0, lowest=0, highest=20)]


@pytest.mark.parametrize("stride", [1, 2, 4, 8])
def test_random_rows_equal_the_model(stride):
    import torch
    N, NT, SMALL = 1_000_000, 5000, 20_000
    rng = np.random.default_rng(1000 + stride)
    lin = random_lineages(rng, NT)
    rows = random_rows(rng, N, stride, NT)
    dev = torch.device("cuda", 0)
    db = api.Database.open(os.path.join(GOLDEN, "toy32"))
    try:
        db.set_lineages(lin)
        dcands = torch.from_numpy(rows.view(np.uint32).reshape(N, stride * 4).view(np.int32)).to(dev)
        out = torch.empty((N, 2), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        db.tally(reset=True)

        def run(n, tally=False, **opt):
            device_vote(db, torch, dcands, n, stride, out, tally=tally, **opt)
            db.synchronize()
            return out[:n].cpu().numpy().view(api.assignment_dtype).reshape(n)

        def model(n, hitmin, hitdiff, lowest, highest):
            return classify_ref.vote_all_fast(lin, rows[:n], hitmin, api.hitdiff_factor(hitdiff), lowest, highest)

        total = np.zeros(NUM_RANKS + 1, dtype=np.uint64)
        per_taxon = np.zeros(int(lin.max()) + 1, dtype=np.uint64)
        for k, opt in enumerate(FULL_SETS):
            got, want = as_triples(run(N, tally=(k < 2), **opt)), model(N, **opt)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, (stride, opt, bad.size, int(bad[0]), rows[bad[0]], got[bad[0]], want[bad[0]])
            assert 0.02 < (want[:, 1] == NUM_RANKS).mean() < (1.0 if opt["hitmin"] >= 40 else 0.98)  # (the rows exercise both outcomes)
            if k < 2:
                total += np.bincount(want[:, 1], minlength=NUM_RANKS + 1).astype(np.uint64)
                per_taxon += np.bincount(want[:, 0][want[:, 0] > 0], minlength=len(per_taxon)).astype(np.uint64)
            if k == 1:                                                       # the host form, on the same rows
                hn = 200_000
                host = db.classify_candidates(rows[:hn], **opt)
                assert np.array_equal(as_triples(host), got[:hn])
        assigned, counts = db.tally()
        assert np.array_equal(assigned, total) and np.array_equal(counts, per_taxon) and int(assigned.sum()) == 2 * N
        # a slice of the rows under every lowest <= highest
        check = classify_ref.vote_all(lin, rows[:300], 5, 0.5, 3, 17)
        assert np.array_equal(check, model(300, 5, 0.5, 3, 17))              # (the fast model is the plain one)
        for lo in range(NUM_RANKS):
            for hi in range(lo, NUM_RANKS):
                opt = dict(hitmin=3, hitdiff=0.6, lowest=lo, highest=hi)
                got, want = as_triples(run(SMALL, **opt)), model(SMALL, **opt)
                assert np.array_equal(got, want), (stride, lo, hi)
        # voters saturate, a stride the rows do not fill, and a single read
        assert np.array_equal(as_triples(run(1, **FULL_SETS[0])), model(1, **FULL_SETS[0]))
    finally:
        db.close()


def test_two_streams_tally_at_the_same_time_and_reset_clears():
    import torch
    N, NT, stride = 1_000_000, 5000, 2
    rng = np.random.default_rng(77)
    lin = random_lineages(rng, NT)
    rows = random_rows(rng, 2 * N, stride, NT)
    rows["tgt"][: N // 2, 0] = rng.integers(0, 10, size=N // 2)             # a quarter of the reads piles onto ten taxa
    dev = torch.device("cuda", 0)
    db = api.Database.open(os.path.join(GOLDEN, "toy32"))
    try:
        db.set_lineages(lin)
        dc = torch.from_numpy(rows.view(np.uint32).reshape(2 * N, stride * 4).view(np.int32)).to(dev)
        outs = [torch.empty((N, 2), dtype=torch.int32, device=dev) for _ in range(2)]
        streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
        torch.cuda.synchronize()
        opt = dict(hitmin=5, hitdiff=0.5, lowest=0, highest=20)
        for rep in range(3):                                                 # enqueued back to back: the two streams' kernels overlap
            for j in range(2):
                db.classify_device(dc[j * N:].data_ptr(), N, stride, out_ptr=outs[j].data_ptr(), stream=streams[j].cuda_stream, tally=True, **opt)
        for s in streams:
            s.synchronize()
        want = classify_ref.vote_all_fast(lin, rows, 5, 0.5, 0, 20)
        for j in range(2):
            got = outs[j].cpu().numpy().view(api.assignment_dtype).reshape(N)
            assert np.array_equal(as_triples(got), want[j * N:(j + 1) * N])
        assigned, counts = db.tally(reset=True)
        assert int(assigned.sum()) == 3 * 2 * N
        assert np.array_equal(assigned, 3 * np.bincount(want[:, 1], minlength=NUM_RANKS + 1).astype(np.uint64))
        assert np.array_equal(counts, 3 * np.bincount(want[:, 0][want[:, 0] > 0], minlength=len(counts)).astype(np.uint64))
        assigned, counts = db.tally()
        assert not assigned.any() and not counts.any()
        # a call without the flag leaves the counters alone
        db.classify_device(dc.data_ptr(), N, stride, out_ptr=outs[0].data_ptr(), **opt)
        assigned, counts = db.tally()
        assert not assigned.any() and not counts.any()
        # new lineages: the device copy follows, and the tallies are sized by the new table
        lin2 = random_lineages(np.random.default_rng(78), 700)
        db.set_lineages(lin2)
        got = as_triples(db.classify_candidates(rows[:50_000], tally=True, **opt))
        assert np.array_equal(got, classify_ref.vote_all_fast(lin2, rows[:50_000], 5, 0.5, 0, 20))
        assigned, counts = db.tally()
        assert int(assigned.sum()) == 50_000 and len(counts) == int(lin2.max()) + 1
    finally:
        db.close()


def test_host_arrays_beyond_one_staged_piece_equal_the_device_path():
    """MC_CLASSIFY_HOST stages 64 MB pieces: 2^20 rows of stride 4; one row more starts a second piece, whose assignments go to
    out + 2^20.  The last row's taxon is one that no other row can be given."""
    import torch
    NT, stride = 5000, 4
    piece = (64 << 20) // (stride * 16)
    n = piece + 1
    rng = np.random.default_rng(4242)
    lin = random_lineages(rng, NT)
    own = NT - 1
    lin[own, 0] = own + 1                                                    # the sequence-level taxon of `own`: only a row whose top candidate is `own` can get it
    rows = random_rows(rng, n, stride, NT)
    rows["tgt"][:, 0][rows["tgt"][:, 0] == own] = 0
    rows[n - 1] = np.zeros(stride, dtype=api.cand_dtype)
    rows[n - 1, 0] = (own, 50, 0, 3)
    opt = dict(hitmin=5, hitdiff=0.5, lowest=0, highest=19)
    dev = torch.device("cuda", 0)
    db = api.Database.open(os.path.join(GOLDEN, "toy32"))
    try:
        db.set_lineages(lin)
        dcands = torch.from_numpy(rows.view(np.uint32).reshape(n, stride * 4).view(np.int32)).to(dev)
        out = torch.empty((n, 2), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        device_vote(db, torch, dcands, n, stride, out, **opt)
        db.synchronize()
        want = as_triples(out.cpu().numpy().view(api.assignment_dtype).reshape(n))
        got = as_triples(db.classify_candidates(rows, **opt))
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (bad.size, int(bad[0]), got[bad[0]], want[bad[0]])
        at = [n - 2, n - 1, 2 ** 20 - 1]
        assert np.array_equal(got[at], classify_ref.vote_all(lin, rows[at], 5, api.hitdiff_factor(0.5), 0, 19))
        assert got[n - 1].tolist() == [own + 1, 0, 1] and (got[: n - 1, 0] != own + 1).all()
    finally:
        db.close()


# ---- composition with the query ----------------------------------------------------------------------------------------------------
def _device_batch(db, reads, dev):
    import torch
    pad = [len(r) + (-len(r)) % 4 for r in reads]
    offs = np.concatenate([[0], np.cumsum(pad)]).astype(np.int64)
    buf = np.zeros(int(offs[-1]) + 16, dtype=np.uint8)
    for r, o in zip(reads, offs[:-1]):
        buf[o:o + len(r)] = np.frombuffer(r, dtype=np.uint8)
    qinfo = np.zeros((len(reads), 4), dtype=np.uint32)
    qinfo[:, 0] = offs[:-1]; qinfo[:, 1] = [len(r) for r in reads]; qinfo[:, 2] = offs[:-1]
    mw = np.array([db.max_windows_in_range(len(r)) for r in reads], dtype=np.int32)
    return (torch.from_numpy(buf).to(dev), torch.from_numpy(qinfo.view(np.int32)).to(dev), torch.from_numpy(mw).to(dev), int(offs[-1]))


@pytest.mark.parametrize("K,lowest", [(2, 0), (3, 4)])
def test_query_then_classify_on_one_stream_equals_the_slot_path(golden, K, lowest):
    import torch
    single, _, _ = golden.reads()
    reads = [r for r in single[:1200] if len(r) > 0]
    opt = dict(hitmin=5, hitdiff=0.5, lowest=lowest, highest=19)
    dev = torch.device("cuda", 0)
    db = api.Database.open(os.path.join(GOLDEN, "toy32"), max_candidates=K)
    try:
        want = db.classify(reads, **opt)                                     # slots + the host form
        assert (want["taxon"] > 0).sum() > 300 and (want["voters"] > 1).sum() > 50
        seq, qi, mw, nch = _device_batch(db, reads, dev)
        n = len(reads)
        side = torch.cuda.Stream(device=dev)
        outs = [torch.empty((n, 2), dtype=torch.int32, device=dev) for _ in range(2)]
        torch.cuda.synchronize()
        # first pipe on the context's own stream, second pipe on a stream of the caller: query and vote back to back, no wait between them
        for j, st in enumerate((0, side.cuda_stream)):
            r = db.query_device(seq.data_ptr(), qi.data_ptr(), n, nch, max_win_ptr=mw.data_ptr(), lowest=lowest, second_pipe=bool(j), stream=st)
            db.classify_device(r.cands, n, K, out_ptr=outs[j].data_ptr(), stream=st, tally=True, **opt)
        db.synchronize(); side.synchronize()
        for j in range(2):
            got = outs[j].cpu().numpy().view(api.assignment_dtype).reshape(n)
            assert np.array_equal(as_triples(got), as_triples(want)), f"pipe {j}"
        assigned, counts = db.tally(reset=True)
        assert int(assigned.sum()) == 2 * n and int(assigned[NUM_RANKS]) == 2 * int((want["taxon"] == 0).sum())
        assert np.array_equal(counts, 2 * np.bincount(want["taxon"][want["taxon"] > 0], minlength=len(counts)).astype(np.uint64))
        assert not db.tally()[0].any()
    finally:
        db.close()
