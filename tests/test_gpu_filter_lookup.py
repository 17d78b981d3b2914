"""GPU: the filter kernel that does the direct-index lookups itself (gw_filter_count_kernel<LOOKUP>, mc_set_tuning "filter_lookup").
The reference's golden reads, singles and pairs, through mc_query_device(MC_DEFER_TAIL) + mc_query_finish as bench.py's timed region
calls them, against the committed expectations; and two tiny synthetic collections whose reads sit on the new kernel's borders
(0 .. 80 features, no hit .. thousands of locations) against the C oracle and against the default order of the kernels on the same
context -- candidates (all four fields) and the per-read statistics (hits, features, found features, lookups)."""
import numpy as np
import pytest

import scale_util
from golden.make_golden import SINGLE_RULES, PAIR_RULES
from metacache_amd import api, synth, synthdb
from test_gpu_parity import cands_equal

pytestmark = pytest.mark.gpu
LANE_HITS = 24                                                  # kernels.hip: MC_LANE_HITS
STRIDE = 112


def _device_batch(reads, mates, insert_max, dev):
    import torch
    both = list(reads) + (list(mates) if mates is not None else [])
    pad = [len(r) + (-len(r)) % 4 for r in both]
    offs = np.concatenate([[0], np.cumsum(pad)]).astype(np.int64)
    buf = np.zeros(int(offs[-1]) + 16, dtype=np.uint8)
    for r, o in zip(both, offs[:-1]):
        buf[o:o + len(r)] = np.frombuffer(r, dtype=np.uint8)
    n = len(reads)
    qinfo = np.zeros((n, 4), dtype=np.uint32)
    qinfo[:, 0] = offs[:n]; qinfo[:, 1] = [len(r) for r in reads]; qinfo[:, 2] = offs[:n]
    l2 = [0] * n
    if mates is not None:
        l2 = [len(m) for m in mates]
        qinfo[:, 2] = offs[n:2 * n]; qinfo[:, 3] = l2
    mw = np.array([(2 + max(len(r) + b, insert_max) // STRIDE) for r, b in zip(reads, l2)], dtype=np.int32)
    return (torch.from_numpy(buf).to(dev), torch.from_numpy(qinfo.view(np.int32)).to(dev), torch.from_numpy(mw).to(dev), int(offs[-1]), n)


def _run(db, batch, K, lowest):
    """one batch as bench.py's timed region runs it -> (cands[n, K, 4] u32, stats[n, 4] u32)"""
    import torch
    seq, qi, mw, nch, n = batch
    dev = seq.device
    r = db.query_device(seq.data_ptr(), qi.data_ptr(), n, nch, max_win_ptr=mw.data_ptr(), lowest=lowest, defer_tail=True)
    db.query_finish()
    out = torch.empty((n, K, 4), dtype=torch.int32, device=dev)
    st = torch.empty((n, 4), dtype=torch.int32, device=dev)
    db.copy_results(out.data_ptr(), r.cands, n * K * 16)
    db.copy_results(st.data_ptr(), r.hit_counts, n * 16)
    db.synchronize()
    return out.cpu().numpy().view(np.uint32), st.cpu().numpy().view(np.uint32)


def _as_cands(row):
    c = np.zeros(len(row), dtype=api.cand_dtype)
    c["tgt"], c["hits"], c["beg"], c["end"] = row[:, 0], row[:, 1], row[:, 2], row[:, 3]
    return c


def _same_rows(a, b):
    """two candidate rows [K, 4] are the same list: the hits of every entry, and all four fields of every entry in use (an unused entry is
    one with hits == 0, include/metacache_amd.h; its other fields are not part of the result)"""
    used = a[:, 1] > 0
    if not used.any():                                           # no candidate at all: both orders write the same defined empty entries
        return np.array_equal(a, b)
    return np.array_equal(a[:, 1], b[:, 1]) and np.array_equal(a[used], b[used])


TIMERS = ("sketch_probe", "probe_cands", "sketch_lane", "gw_filter_count")


@pytest.mark.parametrize("big_min", [None, 0])
@pytest.mark.parametrize("name", ["toy32", "toy16"])
def test_golden_reads_with_the_lookups_in_the_filter_kernel(golden, name, big_min):
    import torch
    dev = torch.device("cuda", 0)
    single, p1, p2 = golden.reads()
    # maxcand 2 (singles and pairs on one context), 3 with taxon merging (singles), 4 with taxon merging (pairs): three contexts
    plans = [(2, [("single", SINGLE_RULES[0]), ("pair", PAIR_RULES[0]), ("pair", PAIR_RULES[1])]),
             (3, [("single", SINGLE_RULES[1])]),
             (4, [("pair", PAIR_RULES[2])])]
    for mc, rules in plans:
        db = api.Database.open(golden.db_path(name), max_candidates=mc, copy_allhits=0)
        assert db.table_layout()["location_bytes"] == 4
        db.set_tuning("direct_index", 1)
        assert db.table_layout()["direct_index"]
        db.set_tuning("filter_lookup", 1)
        if big_min is not None:
            db.set_tuning("big_min", big_min)
        db.timing(True)
        for kind, (rname, rmc, low, ins) in rules:
            assert rmc == mc
            reads, mates = (single, None) if kind == "single" else (p1, p2)
            exp = golden.expected(name, kind + "_" + rname)
            batch = _device_batch(reads, mates, ins, dev)
            db.set_tuning("filter_lookup", 0)
            want, wstat = _run(db, batch, mc, low)                # the default order on the same context: candidates and statistics
            db.set_tuning("filter_lookup", 1)
            db.timing_reset()
            got, gstat = _run(db, batch, mc, low)
            ran = {k: db.timing_get(k)[1] for k in TIMERS}
            assert ran["sketch_lane"] > 0 and ran["gw_filter_count"] > 0 and ran["sketch_probe"] == 0, ran
            for i in range(len(reads)):
                assert cands_equal(_as_cands(got[i]), exp[i][:mc]), (kind, rname, i, got[i], exp[i])
                assert _same_rows(got[i], want[i]), (kind, rname, i, got[i], want[i])
                assert np.array_equal(gstat[i], wstat[i]), (kind, rname, i, gstat[i], wstat[i])
        db.timing(False)
        db.close()


def _border_reads(spec, rng):
    cs = synthdb.CpuSynth()
    pool = []
    for j, L in enumerate((16, 127, 128, 239, 240, 351, 352, 463, 464, 512)):
        for k, sub in enumerate((0.01, 0.06, 0.15)):
            P = synthdb.read_params(spec, 700 + 10 * j + k, read_len=L, sub_rate=sub)
            pool += [bytes(r[:L]) for r in cs.reads(spec, P, 0, 10)]
    src = pool[-1]
    reads = pool + [b"", src[:15], src[:16]]
    reads += [bytes(synth.random_genome(rng, L)) for L in (150, 240, 464)]          # nothing found
    for r in pool[::17]:                                         # N, lower case, junk
        r = bytearray(r)
        for _ in range(3):
            r[int(rng.integers(0, len(r)))] = int(rng.choice(list(b"NnRx-acgu")))
        reads.append(bytes(r))
    return [reads[i] for i in rng.permutation(len(reads))]


@pytest.mark.parametrize("K,lowest,big_min", [(2, 0, None), (4, 0, 0), (2, 4, 0)])
def test_reads_on_the_borders_of_the_lookup_instance(K, lowest, big_min):
    """read lengths 0 .. 512 bp = 0, 16, 32, 48, 64 and 80 features (80: the lookup kernel's reads), collections of 8 and 48 strains
    of one species: no hit, lists a lane of the lookup kernel would finish, the mid / hash kernels' lists, lists the filter finishes,
    lists beyond kGwSmallH.  A run that does not reach every one of those ranges fails."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(77)
    seen = []
    for strains in (8, 48):
        spec = synthdb.phylogeny(1, 1, strains, 20_000, 20_000, seed=9000 + strains, div_strain=(0.002, 0.01))
        db, _ = synthdb.build_database(spec, shards=1, max_candidates=K)
        assert db.table_layout()["location_bytes"] == 4
        db.set_lineages(spec.lineages())
        db.set_tuning("direct_index", 1)
        assert db.table_layout()["direct_index"]
        if big_min is not None:
            db.set_tuning("big_min", big_min)
        reads = _border_reads(spec, rng)
        batch = _device_batch(reads, None, 0, dev)
        db.set_tuning("filter_lookup", 0)
        want, wstat = _run(db, batch, K, lowest)
        db.set_tuning("filter_lookup", 1)
        db.timing(True); db.timing_reset()
        got, gstat = _run(db, batch, K, lowest)
        ran = {k: db.timing_get(k)[1] for k in TIMERS}
        db.timing(False)
        assert ran["sketch_lane"] > 0 and ran["gw_filter_count"] > 0 and ran["sketch_probe"] == 0, ran
        assert ran["probe_cands"] > 0, ran                        # (launched for the reads of more than 64 features)
        db.close()
        odb = scale_util.oracle_database(spec, None, threads=8, with_lineages=True)
        for i, r in enumerate(reads):
            h, e = odb.query(r, b"", K, lowest, 0)
            assert int(gstat[i, 0]) == len(h), (strains, i, len(r), gstat[i], len(h))
            assert cands_equal(_as_cands(got[i]), e), (strains, i, len(r), got[i], e)
            assert _same_rows(got[i], want[i]), (strains, i, len(r), got[i], want[i])
            assert np.array_equal(gstat[i], wstat[i]), (strains, i, len(r), gstat[i], wstat[i])
        odb.close()
        seen.append(gstat[:, 0].astype(np.int64))
    H = np.concatenate(seen)
    print("hit counts: none", int((H == 0).sum()), "1..%d" % LANE_HITS, int(((H >= 1) & (H <= LANE_HITS)).sum()), "65..256", int(((H >= 65) & (H <= 256)).sum()),
          "257..2048", int(((H >= 257) & (H <= 2048)).sum()), "> 2048", int((H > 2048).sum()))
    for lo, hi in ((0, 0), (1, LANE_HITS), (65, 256), (257, 2048), (2049, 1 << 30)):
        assert ((H >= lo) & (H <= hi)).any(), (lo, hi)
