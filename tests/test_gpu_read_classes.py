"""GPU: the lane hand-over (probe_cands_one) and every read class of an ordinary query -- mid_cands_kernel<4 / 8 / 16>,
hash_cands_kernel<9 / 10 / 11>, the filtered path (compact store: as far as the classification; 8-byte store: big_filter_kernel's two
instances, big_count_kernel's two), the wave kernels (query_kernel, sort_candidates_kernel, wave_rejoin_kernel) and the chunk lanes'
own rule -- at their borders, through db.query on tables of chosen lists (tests/class_lists.py; the inputs are proved in
tests/test_class_lists_cpu.py).  Whatever kernel finishes a read, its candidates must be the oracle's on the sorted union of the
lists of its features: exact integer equality, plus the per-read counts, the batch statistics and the launched timers against the
model.  One context per (store, max_candidates, sketch length), made once per module."""
import numpy as np
import pytest

import class_lists as cl

pytestmark = pytest.mark.gpu

COMBOS = [(1, 0), (2, 0), (4, 0), (1, cl.TAX_RANK), (2, cl.TAX_RANK), (4, cl.TAX_RANK)]
SETS = ("handover", "classes", "mid", "hash", "wave", "big", "tandem", "chunk")
REACHED = {cl.COMPACT: {}, cl.WIDE8: {}}                      # the union over the file's batches (the last test reads it)


def note(store, reached):
    for k, v in reached.items():
        if k != "filter>uncertain":                              # (a case in a batch at another big_min than its own)
            REACHED[store][k] = REACHED[store].get(k, 0) + v


@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(2026)
    w = dict(db={})
    w[16] = dict(handover=cl.handover_cases(rng), classes=cl.class_cases(rng), mid=cl.mid_cases(rng), hash=cl.hash_cases(rng), wave=cl.wave_cases(rng),
                 big=cl.big_cases(rng), tandem=cl.tandem_cases(rng), chunk=cl.chunk_cases(rng), filler=cl.lane_filler(rng, 130),
                 lead=cl.lane_filler(rng, 2, shape="single100"))
    w["full"] = cl.full_list_cases(rng)
    w[16]["full"] = [c for v in w["full"].values() for c in v]
    for s in (8, 15):
        w[s] = dict(handover=cl.handover_cases(rng, s), filler=cl.lane_filler(rng, 6, s), lead=cl.lane_filler(rng, 2, s, shape="single100"),
                    chunk=cl.chunk_cases(rng, s))

    def db(store, K, s=16, allhits=0):
        key = (store, K, s, allhits)
        if key not in w["db"]:
            w["db"][key] = cl.context([c for v in w[s].values() for c in v], store, K, s, copy_allhits=allhits)
        return w["db"][key]
    w["ctx"] = db
    yield w
    for d in w["db"].values():
        d.close()


def one_route(c, store, big_min):
    route = cl.route_of(c, store, big_min)
    return route + ">" + cl.big_route(c) if route == "filter" and store == cl.WIDE8 else route


def by_big_min(cases):
    out = {}
    for c in cases:
        out.setdefault(cl.case_big_min(c), []).append(c)
    return sorted(out.items())


@pytest.mark.parametrize("K,lowest", COMBOS)
@pytest.mark.parametrize("store", cl.STORES)
@pytest.mark.parametrize("which", SETS)
def test_borders_against_the_oracle(world, which, store, K, lowest):
    """every set of border cases, each batch at the big_min its cases name; the route every case was built for is the model's
    (asserted on the CPU), and a batch's kernels are the ones of its routes"""
    db = world["ctx"](store, K)
    for big_min, cases in by_big_min(world[16][which]):
        r = cl.check(db, cases, K, lowest, store, big_min)
        note(store, r)
        for c in cases:
            want = cl.named_route(c, store)
            assert want is None or want in r or (want == "filter" and any(k.startswith("filter>") for k in r)), (c.name, want, r)
        # the reads of ONE route alone: the host launches a class's kernel only where its counter is non-zero, so the timers of such a
        # batch say which kernel took its reads
        if len(r) > 1:
            for route in r:
                alone = [c for c in cases if one_route(c, store, big_min) == route]
                assert set(cl.check(db, alone, K, lowest, store, big_min)) == {route}


@pytest.mark.parametrize("fusion", [0, 1])
@pytest.mark.parametrize("quad", [0, 1])
@pytest.mark.parametrize("s", [16, 8, 15])
@pytest.mark.parametrize("store", cl.STORES)
def test_hand_over(world, store, s, quad, fusion):
    """the hand-over's borders at sketch length 16 (paired stores, wide fetch, sort16's emit), 8 (the other emit) and 15 (scalar
    fetch; behind ONE read of one window every fbase is odd: single stores), lane-private and quad-cooperative lookups, sketching
    and probing in one kernel and in two"""
    db = world["ctx"](store, 2, s)
    cases = world[s]["handover"] + world[s]["filler"]
    tuning = dict(quad_lookup=quad, lane_fusion=fusion)
    for lead in ([], world[s]["lead"][:1]):
        batch = lead + cases
        parity = {int(f) & 1 for f in cl.first_slots(batch)[len(lead):]}
        assert parity == ({1} if lead and s == 15 else {0}), (s, parity)
        for lowest in (0, cl.TAX_RANK):
            note(store, cl.check(db, batch, 2, lowest, store, cl.NO_FILTER, tuning=tuning))
        stay = [c for c in batch if not c.handed]                # H up to kLaneHits alone: no class kernel may run (check holds the timers)
        assert any(c.H == cl.LANE_HITS for c in stay) and set(cl.check(db, stay, 2, 0, store, cl.NO_FILTER, tuning=tuning)) == {"lane"}
    if s == 15:                                                  # (273 windows x 15 = 4095 feature slots: chunk_finish_kernel's border from below)
        note(store, cl.check(db, world[15]["chunk"], 2, 0, store, 0, tuning=tuning))


def one_of_each(w16):
    """one case per class (and its big_min)"""
    by = {c.name: c for v in w16.values() for c in v}
    names = ["kLaneHits + 1 entries: over, odd", "mid<8>: 33 entries, H 128", "mid<16>: 65 entries, H 256", "hash256: 65 entries", "hash512: per 6, H 321",
             "hash1024: 128 entries", "big_min 128: H 129", "big: 65 entries", "H 1025, maxWin 9"]
    return [by[n] for n in names]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129])
@pytest.mark.parametrize("store", cl.STORES)
def test_position_in_the_batch(world, store, n):
    """a case of every class at read 0, in the middle and at the last read of batches around the lane kernel's block (kLaneBlock 128)
    and wave (64); the other reads finish in the lane, so only the one class's kernel runs (check holds the timers against that)"""
    db = world["ctx"](store, 2)
    filler = world[16]["filler"]
    for i, c in enumerate(one_of_each(world[16])):
        for pos in sorted({0, n // 2, n - 1}):
            batch = filler[:pos] + [c] + filler[pos:n - 1]
            assert len(batch) == n and batch[pos] is c
            r = cl.check(db, batch, 2, cl.TAX_RANK if (i + pos) % 2 else 0, store, cl.case_big_min(c))
            assert set(r) - {"lane"} and len(set(r) - {"lane"}) == 1 and r.get("lane", 0) == n - 1, r
            note(store, r)


@pytest.mark.parametrize("cls", ["mid64", "mid128", "mid256"])
@pytest.mark.parametrize("store", cl.STORES)
def test_a_read_for_every_group_of_the_grid(world, store, cls):
    """mid_cands_kernel<G>: 256 / G reads of the class give every group of a block its read; one fewer and one more leave idle groups
    (rec.z == 0) in the first and in a second block"""
    cases = world["full"][cls]
    full = len(cases) - 1
    assert full == {"mid64": 64, "mid128": 32, "mid256": 16}[cls]
    for n in (full - 1, full, full + 1):
        for lowest in (0, cl.TAX_RANK):
            r = cl.check(world["ctx"](store, 2), cases[:n], 2, lowest, store, cl.NO_FILTER)
            assert r == {cls: n}, r
            note(store, r)


@pytest.mark.parametrize("K,lowest", [(1, 0), (2, cl.TAX_RANK), (4, 0), (4, cl.TAX_RANK)])
@pytest.mark.parametrize("store", cl.STORES)
def test_every_class_in_one_batch(world, store, K, lowest):
    """all cases of sketch length 16 in one batch in random order, at the default big_min and at 0"""
    rng = np.random.default_rng(K + lowest)
    cases = [c for k, v in world[16].items() for c in v]
    for big_min in (cl.BIG_MIN_DEFAULT, 0, cl.NO_FILTER):
        batch = [cases[i] for i in rng.permutation(len(cases))]
        r = cl.check(world["ctx"](store, K), batch, K, lowest, store, big_min)
        note(store, r)
        if big_min == cl.BIG_MIN_DEFAULT:
            want = {"lane", "mid64", "hash256"} | ({"filter"} if store == cl.COMPACT else {"filter>count", "filter>count2", "filter>wave", "wave"})
            assert want <= set(r), r
        if big_min == cl.NO_FILTER:
            assert {"lane", "mid64", "mid128", "mid256", "hash256", "hash512", "hash1024", "wave", "chunk>wave", "sketch>wave"} == set(r), r


@pytest.mark.parametrize("how", ["lane_path 0", "K 5"])
@pytest.mark.parametrize("store", cl.STORES)
def test_wave_kernels(world, store, how):
    """the same tables without the lane path, and with more candidates than a lane keeps: query_kernel (kFuseCap: candidates inside
    the kernel for lists up to 32, without taxon merging) and sort_candidates_kernel (kLdsCap: LDS up to 256, a segment in HBM
    beyond) finish every read"""
    K = 5 if how == "K 5" else 2
    db = world["ctx"](store, K)
    cases = [c for k in ("wave", "handover", "classes", "tandem", "filler") for c in world[16][k]][:150]
    assert {cl.FUSE_CAP, cl.FUSE_CAP + 1, cl.LDS_CAP, cl.LDS_CAP + 1} <= {c.H for c in cases}
    for lowest in (0, cl.TAX_RANK):
        r = cl.check(db, cases, K, lowest, store, cl.BIG_MIN_DEFAULT, lane_path=(how != "lane_path 0"))
        assert set(r) == {"wave"}, r
        note(store, {"wave (no lane path)": len(cases)})


@pytest.mark.parametrize("store", cl.STORES)
def test_wave_kernels_return_the_sorted_lists(world, store):
    """copy_allhits: the lists that come back are the sorted unions, for H at kLdsCap and one more among the rest"""
    db = world["ctx"](store, 2, 16, allhits=1)
    cases = world[16]["wave"] + world[16]["handover"] + world[16]["tandem"]
    assert {cl.LDS_CAP, cl.LDS_CAP + 1} <= {c.H for c in cases}
    r = cl.check(db, cases, 2, 0, store, cl.BIG_MIN_DEFAULT, allhits=True)
    assert set(r) == {"wave"}, r


@pytest.mark.parametrize("store", cl.STORES)
def test_the_longest_list_a_read_may_have(store):
    """a table of its own (two lists of a million locations): H == kMaxHitsPerQuery has candidates, one location more has none"""
    rng = np.random.default_rng(99)
    cases = cl.max_hits_cases(rng) + cl.lane_filler(rng, 3)
    assert [c.H for c in cases[:2]] == [cl.MAX_HITS, cl.MAX_HITS + 1]
    db = cl.context(cases, store, 2, 16, max_queries=16)
    try:
        for lowest in (0, cl.TAX_RANK):
            r = cl.check(db, cases, 2, lowest, store, 0)
            assert r == {"chunk>wave": 1, "too_many": 1, "lane": 3}, r
            note(store, r)
    finally:
        db.close()


def test_every_class_was_reached():
    """the union over the file's batches: every work list of read_class.h, the filtered class, the wave class, the chunk rule, on the
    stores where each exists (the file's last test: it needs every test above to have run)"""
    both = {"lane", "mid64", "mid128", "mid256", "hash256", "hash512", "hash1024", "wave", "chunk>wave", "sketch>wave", "too_many", "wave (no lane path)"}
    want = {cl.COMPACT: both | {"filter", "chunk>filter", "sketch>filter"}, cl.WIDE8: both | {"filter>count", "filter>count2", "filter>wave"}}
    for store in cl.STORES:
        assert set(REACHED[store]) == want[store], (store, sorted(want[store] ^ set(REACHED[store])))
