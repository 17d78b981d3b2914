"""GPU: the shape-fixed instances of gw_filter_count_kernel<LOOKUP> (window range 2 or 3 for all reads, 1 or 2 candidates: the frame, the
neighbour windows and the K rounds are constants of their code, the winners' bounds and step D's lists are sized by K) and the host rule
that picks them (lookup_shape, csrc/query_rules.h).

The collection is groups of IDENTICAL strains as in test_gpu_filter_lookup_room.py (1, 20, 40 and 100 strains of 4 kbp: a feature's list
has as many locations as its group has strains) and twelve identical strains of 130 kbp, whose windows lie up to 1 160 apart -- farther than
the gap between two targets' window numbers.  Batches are handed over with ONE window range for all reads (max_win_uniform, as bench.py does),
so a batch holds reads of one range only: 40 .. 111 bp (range 2) and 112 .. 223 bp (range 3).  Every shape is asserted from the oracle's
sketch, lists and hits before anything runs on the device:

  * hits exactly D and D + 1 windows apart (D = range - 1: inside one window range, and just outside);
  * hits on both sides of a block border of the filter (window numbers = 254, 255, 0, 1 mod 256), some reads with 255 and 0 in one target;
  * fewer than K candidates of two hits (step D fills the places from single hits), with none and with one strong candidate;
  * two best ranges in ONE target (two pieces of a 130 kbp strain, more than 1 024 windows apart, with equal hits: the exact wave kernel);
  * more than 384 kept numbers (phase B repeated into the pool);
  * two species with two hits each (taxon merging finishes the read in the kernel), no hit, a lane's list.

`filter_lookup` 1 against 0 on one context (candidates and all four statistics words), every read against the C oracle, with and without taxon
merging, maxcand 1, 2 and 3; which instance the rule picked is read from the launch counters.  A uniform range of 1 is no range the
reference computes for any read (2 + length / stride), so that batch -- the unfixed instance, like maxcand 3 -- is compared with the other
order of the kernels and with the oracle's hit counts only."""
import numpy as np
import pytest

import cpuref
import scale_util
from metacache_amd import synth, synthdb
from test_gpu_filter_lookup import TIMERS, _as_cands, _device_batch, _same_rows
from test_gpu_filter_lookup_entries import KEEP, STRIDE, gw_bases, route_of, shape_of
from test_gpu_parity import cands_equal

pytestmark = pytest.mark.gpu
LEN, LONG = 36 * STRIDE, 130_000
GROUPS = ((1, LEN), (20, LEN), (40, LEN), (100, LEN), (12, LONG))   # (identical strains, length)
INSTANCES = ("gw_filter_lookup_w3_k2", "gw_filter_lookup_w3_k1", "gw_filter_lookup_w2_k2", "gw_filter_lookup_w2_k1", "gw_filter_lookup_any")


class World:
    pass


def instance_name(uniform, K):
    """the host rule (lookup_shape; its CPU test: test_lookup_shape_cpu.py) as the launch counters name it"""
    return f"gw_filter_lookup_w{uniform}_k{K}" if uniform in (2, 3) and K in (1, 2) else "gw_filter_lookup_any"


def collection():
    parts = [synthdb.phylogeny(1, 1, m, n, n, seed=8100 + m, div_strain=(0.0, 0.0)) for m, n in GROUPS]
    group = np.concatenate([np.full(len(p.targets), i, dtype=np.int64) for i, p in enumerate(parts)])
    first = np.cumsum([0] + [len(p.targets) for p in parts])
    spec = synthdb.Phylogeny(np.concatenate([p.targets for p in parts]), group, group.copy(), len(parts), len(parts))
    return spec, {m: int(first[i]) for i, (m, _) in enumerate(GROUPS)}


def build_world():
    """CPU only: the collection, the oracle's database and the reads of both ranges, each kind found by its shape"""
    w = World()
    w.spec, first = collection()
    cs = synthdb.CpuSynth()
    genome = {m: cs.target(w.spec, t) for m, t in first.items()}
    for (m, _), t in zip(GROUPS, first.values()):
        assert np.array_equal(cs.target(w.spec, t + m - 1), genome[m]), m
    orc = cpuref.oracle()
    w.odb = odb = scale_util.oracle_database(w.spec, None, threads=8, with_lineages=True)
    lengths = w.spec.targets["length"].astype(np.int64)
    w.bases = bases = gw_bases([range(int(n)) for n in lengths])
    memo, shapes = {}, {}

    def oracle(read, K, lowest):
        if (read, K, lowest) not in memo:
            memo[read, K, lowest] = odb.query(read, b"", K, lowest, 0)
        return memo[read, K, lowest]

    def shape(read):
        if read not in shapes:
            mw = 2 + len(read) // STRIDE
            sh = shape_of(orc, odb, bases, read, b"", mw)
            feats, counts = orc.sketch(read)
            sizes = [len(odb.lookup(int(f))) for i in range(len(feats)) for f in feats[i, :counts[i]]]
            sh["sizes"] = [n for n in sizes if n]
            h, _ = oracle(read, 1, 0)
            tg = h["tgt"].astype(np.int64)
            sh["gw"] = bases[tg] + h["win"].astype(np.int64)
            sh["wins"] = {int(t): sorted(set(h["win"][tg == t].tolist())) for t in set(tg.tolist())}
            sh["routes"] = {K: route_of(sh, bases, K, False, mw) for K in (1, 2, 3)} if sh["H"] else {K: "8-none" for K in (1, 2, 3)}
            shapes[read] = sh
        return shapes[read]

    rng = np.random.default_rng(311)

    def cut(m, start, n):
        return bytes(genome[m][start:start + n])

    def junk(n):
        return bytes(synth.random_genome(rng, n))

    def find(cands, ok, what, count=1):
        out = []
        for r in cands:
            if ok(shape(r)):
                out.append(r)
                if len(out) == count:
                    return out
        raise AssertionError(f"{len(out)} of {count} reads for: {what}")

    w.reads, w.kinds = {}, {}
    for rng_, (lo, hi) in ((2, (40, 111)), (3, (112, 223))):
        D, L = rng_ - 1, hi - 3
        half = L // 2
        own = lambda s: s["H"] > 64 and s["routes"][2] in ("1", "2")
        kinds = {}
        kinds["own"] = find((bytes(synth.mutate(rng, genome[20][o:o + n], 0.01 * (i % 3 == 2))) for i, (o, n) in
                             enumerate((int(rng.integers(0, LEN - hi)), int(rng.integers(lo + 20, hi + 1))) for _ in range(60))), own, "the kernel's own reads", 12)
        # two pieces of one strain whose hits lie in exactly two windows, d apart
        def apart(d):
            def ok(s):
                wins = list(s["wins"].values())
                return own(s) and len(wins) == 20 and all(len(x) == 2 and x[1] - x[0] == d for x in wins)
            pl = min(half, 60)                                       # (a piece lies inside ONE window of its strain)
            return find((cut(20, j * STRIDE + a, pl) + cut(20, (j + d) * STRIDE + a, pl) for j in range(1, 30) for a in (8, 20, 32, 44)), ok, f"hits {d} windows apart", 3)
        kinds["apart_D"], kinds["apart_D1"] = apart(D), apart(D + 1)
        # the filter's block border: a target's hits in windows numbered 255 and 0 (mod 256)
        def straddles(s):
            both = any({255, 0} <= {int(bases[t] + x) % 256 for x in wins} for t, wins in s["wins"].items())
            return own(s) and both
        kinds["border"] = find((cut(m, j * STRIDE + a, n) for m in (20, 40) for n in (lo + 10, L) for j in range(0, 33) for a in (0, 30, 60, 90)), straddles, "255 and 0 mod 256 in one target", 2)
        for x in (254, 1):                                           # ... and the numbers next to the border
            kinds[f"border_{x}"] = find((cut(m, j * STRIDE + a, n) for m in (20, 40) for n in (lo + 10, L) for j in range(0, 33) for a in (0, 30, 60, 90)),
                                        lambda s, x=x: own(s) and (s["gw"] % 256 == x).any(), f"a hit in a window numbered {x} mod 256", 1)
        kinds["many"] = find((cut(40, j * STRIDE + a, L) for j in range(0, 33) for a in (0, 1, 2, 5)), lambda s: s["kept"] > KEEP + 24 and s["H"] <= 2048 and s["rounds"] <= 128, "more than 384 kept numbers", 2)
        pad = lambda r: r + junk(max(0, lo + 8 - len(r)))
        one = [pad(cut(100, o, n)) for o in range(0, LEN - 40, 11) for n in (18, 22, 26)]
        kinds["single_hits"] = find(one, lambda s: s["sizes"] == [100] and s["routes"][2] == "2", "one list, no candidate of two hits", 2)
        lone = [cut(1, o, 44) for o in range(0, LEN - 44, 13)]
        kinds["one_strong"] = find((pad(a + b) for a in lone[:60] for b in one[:40:3] if len(a + b) <= hi), lambda s: sorted(s["sizes"])[-1] == 100 and sorted(s["sizes"])[:-1] == [1] * (len(s["sizes"]) - 1)
                                   and len(s["sizes"]) >= 3 and s["routes"][2] == "2" and max(map(len, s["wins"].values())) == 1, "one candidate of two hits, single hits beside it", 2)
        far = [cut(12, j * STRIDE + 8, half) + cut(12, (j + 1030 + k) * STRIDE + 8, half) for j in range(2, 100, 3) for k in range(0, 100, 9)]
        kinds["again"] = find(far, lambda s: s["routes"][2] == "4", "two best ranges in one target", 2)
        kinds["two_species"] = find((pad(cut(20, j * STRIDE + 8, 48) + cut(1, j * STRIDE + 8, 60)) for j in range(1, 30)),
                                    lambda s: s["H"] > 64 and s["kept"] <= KEEP - 24, "two species", 3)
        kinds["none"] = [junk(L)]
        kinds["lane"] = find((cut(1, o, L) for o in range(0, LEN - L, 50)), lambda s: 1 <= s["H"] <= 24, "a lane's list", 1)
        for r in kinds["two_species"]:
            _, e = oracle(r, 2, 4)
            assert len(e) == 2 and (e["hits"] >= 2).all(), e
        reads = [r for k in kinds.values() for r in k]
        assert all(lo <= len(r) <= hi for r in reads), sorted(map(len, reads))
        res = np.concatenate([shape(r)["gw"] % 256 for r in reads])
        assert all((res == x).any() for x in (254, 255, 0, 1))
        w.reads[rng_] = [reads[i] for i in rng.permutation(len(reads))] * 3     # (a wave of the smallest grid walks several of them)
        w.kinds[rng_] = kinds
    w.oracle, w.shape = oracle, shape
    return w


@pytest.fixture(scope="module")
def world():
    w = build_world()
    yield w
    w.odb.close()


def _run(db, batch, K, lowest, uniform):
    """one batch as bench.py's timed region runs it, ONE window range for all reads -> (cands[n, K, 4] u32, stats[n, 4] u32)"""
    import torch
    seq, qi, _, nch, n = batch
    r = db.query_device(seq.data_ptr(), qi.data_ptr(), n, nch, max_win_uniform=uniform, lowest=lowest, defer_tail=True)
    db.query_finish()
    out = torch.empty((n, K, 4), dtype=torch.int32, device=seq.device)
    st = torch.empty((n, 4), dtype=torch.int32, device=seq.device)
    db.copy_results(out.data_ptr(), r.cands, n * K * 16)
    db.copy_results(st.data_ptr(), r.hit_counts, n * 16)
    db.synchronize()
    return out.cpu().numpy().view(np.uint32), st.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("lowest", [0, 4])                           # 4: candidates merged at a taxon rank -- the instances' twins
@pytest.mark.parametrize("K", [1, 2, 3])
def test_fixed_instances_against_the_other_order_and_the_oracle(world, K, lowest):
    import torch
    dev = torch.device("cuda", 0)
    for rng_ in (2, 3):                                              # every kind is where it is meant to be (asserted when it was found)
        routes = [world.shape(r)["routes"][2] for r in world.reads[rng_]]
        assert {"1", "2", "4", "7"} <= set(routes), set(routes)
    db, _ = synthdb.build_database(world.spec, shards=1, max_candidates=K)
    try:
        assert db.table_layout()["location_bytes"] == 4
        db.set_lineages(world.spec.lineages())
        db.set_tuning("direct_index", 1)
        assert db.table_layout()["direct_index"]
        db.set_tuning("big_min", 0)
        db.set_tuning("filter_bpc", 1)
        for uniform, rng_ in ((3, 3), (2, 2), (1, 2)):
            reads = world.reads[rng_]
            for order in (reads, reads[::-1]):
                batch = _device_batch(order, None, 0, dev)
                db.set_tuning("filter_lookup", 0)
                want, wstat = _run(db, batch, K, lowest, uniform)
                db.set_tuning("filter_lookup", 1)
                db.timing(True); db.timing_reset()
                got, gstat = _run(db, batch, K, lowest, uniform)
                ran = {k: db.timing_get(k)[1] for k in TIMERS + INSTANCES}
                db.timing(False)
                assert ran["sketch_lane"] > 0 and ran["gw_filter_count"] > 0 and ran["sketch_probe"] == 0, ran
                picked = [k for k in INSTANCES if ran[k]]
                assert picked == [instance_name(uniform, K)], (uniform, K, ran)
                assert np.array_equal(gstat, wstat), np.flatnonzero((gstat != wstat).any(axis=1))[:8]
                for i, r in enumerate(order):
                    assert _same_rows(got[i], want[i]), (uniform, i, len(r), got[i], want[i])
                    h, e = world.oracle(r, K, lowest)
                    assert int(gstat[i, 0]) == len(h), (uniform, i, len(r), gstat[i], len(h))
                    if uniform == rng_:
                        assert cands_equal(_as_cands(got[i]), e[:K]), (uniform, i, len(r), got[i], e)
    finally:
        db.close()
