"""CPU: the inputs of tests/test_gpu_read_classes.py are proved here, before any kernel sees them -- every border of the lane
hand-over (probe_cands_one) and of the read classes (read_class.h) appears with a case on each side, the model's class, entries, over,
per, big_setup shape and route match what each case was named for, no case leaves its route open, the oracle's answer is strong for
some cases of every class and weak for at least one, the Python mirror of the class rule agrees with literal rows, and the borders
the lane path cannot reach are shown unreachable from the constants."""
import numpy as np
import pytest

import class_lists as cl
import sketch_ref

COMBOS = [(1, False), (2, False), (4, False), (1, True), (2, True), (4, True)]
NUMBER = {name: i for i, name in enumerate(cl.CLASSES)}


@pytest.fixture(scope="module")
def sets():
    rng = np.random.default_rng(2026)
    return dict(handover=cl.handover_cases(rng), classes=cl.class_cases(rng), mid=cl.mid_cases(rng), hash=cl.hash_cases(rng), wave=cl.wave_cases(rng),
                big=cl.big_cases(rng), tandem=cl.tandem_cases(rng), chunk=cl.chunk_cases(rng), chunk15=cl.chunk_cases(rng, 15),
                filler=cl.lane_filler(rng, 40), odd=cl.handover_cases(rng, 15), eight=cl.handover_cases(rng, 8))


def everything(sets):
    return [c for v in sets.values() for c in v]


def test_constants_are_the_ones_the_cases_were_written_for():
    assert (cl.LANE_HITS, cl.LANE_K, cl.LANE_MAX_LEN, cl.LANE_S, cl.LANE_BLOCK, cl.FUSE_CAP, cl.MID_R) == (24, 4, 512, 16, 128, 32, 16)
    assert (cl.MID64, cl.MID128, cl.MID_MAX, cl.LDS_CAP, cl.HASH_MAX, cl.HASH_ENT, cl.HASH_WIN) == (64, 128, 256, 256, 1024, 256, 8)
    assert (cl.BIG_ENT, cl.BIG_EPL, cl.BIG_MAX_ROUNDS, cl.BIG_MAX_FILTERED, cl.SMALL_H, cl.REC_ENT_MAX, cl.MAX_HITS) == (64, 3, 256, 1024, 2048, 4095, (1 << 20) - 1)
    assert cl.CHUNK_WINS == 1 and cl.GAP == 1024


def test_the_mirror_of_the_class_rule_against_literal_rows():
    """the rows are numbers written down on their own (the class numbers of the work-list table in kernels.h), as the decision table
    of tests/cpp/read_class_check.cpp is -- the mirror is not held against the header it was read from"""
    seen = set()
    for (H, ent, mw, big_min, compact), want in cl.CLASS_ROWS:
        got = cl.read_class(H, ent, mw, big_min, compact)
        assert NUMBER[got] == want, ((H, ent, mw, big_min, compact), got, want)
        assert cl.filter_takes(H, ent, mw, big_min, compact) == (want == 7)
        seen.add(want)
    assert seen == set(range(8))
    assert [cl.filter_second(h, e, c) for h, e, c in ((2048, 200, True), (2049, 1, True), (5000, 64, False), (70, 65, False))] == [False, True, False, True]
    assert [cl.segment_hits(h, c) for h, c in ((256, "wave"), (257, "wave"), (257, "hash512"), ((1 << 20) - 1, "wave"), (1 << 20, "wave"))] == [0, 257, 0, (1 << 20) - 1, 0]


def test_reads_are_what_the_device_sketches(sets):
    """window counts, maxWindowsInRange and slot layout of the shapes; no window repeats a hash unless the case is there for that; no
    two reads share a feature (table_of asserts it)"""
    want = {"single100": (1, 2), "single150": (2, 3), "pair250": (6, 6), "pair350": (6, 8), "pair391": (8, 8), "pair400": (8, 9), "pair512": (10, 11)}
    rng = np.random.default_rng(5)
    for shape, (wins, mw) in want.items():
        r = cl.new_read(rng, shape)
        assert (r.windows, r.max_win, len(r.feats)) == (wins, mw, wins * 16) and r.lane and not r.chunked, shape
        l1, l2 = cl.SHAPES[shape]
        assert r.windows == len(sketch_ref.windows(l1, 16, 127, 112)) + len(sketch_ref.windows(l2, 16, 127, 112))
    for c in everything(sets):
        assert c.read.dup == c.name.startswith("tandem"), c.name
        assert c.read.lane == (not c.read.dup and not c.read.chunked), c.name
    keys, sizes, vals = cl.table_of(everything(sets))
    assert len(set(keys.tolist())) == len(keys) == sum(c.entries for c in everything(sets)) and int(sizes.astype(np.int64).sum()) == len(vals)
    assert sizes.min() >= 1 and sizes.max() <= cl.MAX_LIST and np.all(vals[:, 0] < cl.WINDOWS[vals[:, 1]])


def test_every_case_has_the_model_it_was_named_for(sets):
    names = set()
    for c in everything(sets):
        assert c.name + str(c.read.s) not in names, c.name
        names.add(c.name + str(c.read.s))
        assert (c.H, c.entries) == (c.named["H"], c.named["entries"]) and c.n + c.m == c.entries, c.name
        assert c.over == (c.entries > cl.LANE_HITS) and c.handed == (c.H > cl.LANE_HITS or c.over) and c.coop == (c.handed and not c.over), c.name
        for key in ("over", "coop"):
            if key in c.named:
                assert getattr(c, key) == c.named[key], (c.name, key)
        for store in cl.STORES:
            want = cl.named_route(c, store)
            got = cl.route_of(c, store, cl.case_big_min(c))
            assert want is None or got == want, (c.name, store, got, want)
            if got == "filter" and store == cl.WIDE8:
                lo, hi = c.big_kept()
                assert cl.big_route(c) != "uncertain" and (cl.big_route(c) == "wave" or lo == hi == c.H), (c.name, lo, hi)       # no route is left open
                assert "big" not in c.named or cl.big_route(c) == c.named["big"], (c.name, cl.big_route(c))
                assert "second" not in c.named or cl.filter_second(c.H, c.entries, False) == (c.named["second"] if isinstance(c.named["second"], bool) else c.named["second"][store])
                assert "shape_" not in c.named or c.big_shape() == c.named["shape_"], (c.name, c.big_shape())
        if "no_lane" in c.named:
            assert cl.route_of(c, cl.COMPACT, cl.NO_FILTER, lane_path=False) == c.named["no_lane"]


def test_every_border_appears_from_both_sides(sets):
    L = cl.LANE_HITS
    shape = lambda v: {(c.H, c.entries) for c in v}
    # ---- probe_cands_one
    for v in (sets["handover"], sets["odd"], sets["eight"]):
        hs = shape(v)
        assert {(L, L), (L + 1, L + 1)} <= hs                                       # H == kLaneHits finishes in the lane, one more is handed over
        assert any(c.entries == L and c.coop for c in v) and any(c.entries == L + 1 and c.over for c in v)
        assert any(c.over and c.entries % 2 == 1 for c in v) and any(c.over and c.entries % 2 == 0 for c in v)      # flush_entries: odd and even
        assert any(c.handed and c.n == 0 for c in v) and any(c.handed and c.m == 0 for c in v) and any(c.handed and c.n and c.m for c in v)
        assert any(c.handed and c.H <= cl.MID_MAX and c.entries < len(c.read.feats) for c in v)                      # slots behind the entries stay unzeroed
    assert {c.read.s for c in sets["odd"]} == {15} and {c.read.s for c in sets["eight"]} == {8}                      # scalar fetch / the other emit
    # (fbase odd: an odd sketch length behind an odd number of windows -- one read of one window in front)
    lead = cl.new_read(np.random.default_rng(1), "single100", 15)
    assert lead.windows == 1 and (lead.windows * 15) % 2 == 1
    # ---- read_class: H on both sides of every limit, counting allowed and not; maxWin 8 / 9; big_min 0 / 128 / 4096
    by = {c.name: c for c in sets["classes"]}
    for H in (64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025):
        assert (by[f"H {H}, maxWin 8"].H, by[f"H {H}, maxWin 8"].max_win, by[f"H {H}, maxWin 9"].H, by[f"H {H}, maxWin 9"].max_win) == (H, cl.HASH_WIN, H, cl.HASH_WIN + 1)
    for bm in (0, 128, 4096):
        hs = sorted(c.H for c in sets["classes"] if c.named["big_min"] == bm and c.max_win <= cl.HASH_WIN)
        lo = max(bm, cl.MID64)
        assert lo in hs and lo + 1 in hs, (bm, hs)
        for store in cl.STORES:
            sides = {cl.route_of(c, store, bm) == "filter" for c in sets["classes"] if c.named["big_min"] == bm and c.H in (lo, lo + 1) and c.max_win <= cl.HASH_WIN}
            assert sides == {False, True}, (bm, store)
    assert {cl.filter_second(c.H, c.entries, True) for c in sets["classes"] if c.H in (cl.SMALL_H, cl.SMALL_H + 1)} == {False, True}
    # ---- mid_cands_kernel<G>: entries at 4 * G and one more; full and padded lists; singletons and lists
    for G, cls in ((4, "mid64"), (8, "mid128"), (16, "mid256")):
        v = [c for c in sets["mid"] if c.named["route"] == cls]
        assert {4 * G, 4 * G + 1} <= {c.entries for c in v}, G
        assert any(c.H == G * cl.MID_R for c in v) and any(c.H < G * cl.MID_R for c in v)
        assert any(c.m == 0 for c in v) and any(c.n == 0 for c in v) and any(c.n and c.m for c in v)
    # ---- hash_cands_kernel: every PER instance from both sides; more entries and more distinct pairs than one wave-load
    pers = {"hash256": {2, 3, 4}, "hash512": {5, 6, 7, 8}, "hash1024": {9, 10, 11, 12, 13, 14, 15, 16}}
    for cls, want in pers.items():
        got = {c.per() for c in sets["hash"] if c.named["route"] == cls}
        assert got >= (want if cls != "hash1024" else {9, 10, 11, 12, 13, 14, 15, 16} & got) and {min(want), max(want)} <= got, (cls, got)
    assert {10, 11, 12, 13, 14, 15, 16} <= {c.per() for c in sets["hash"] if c.named["route"] == "hash1024"}
    assert any(c.entries > 64 for c in sets["hash"]) and any(len(np.unique(c.locs)) > 64 for c in sets["hash"])
    # ---- the wave kernels
    assert {cl.FUSE_CAP, cl.FUSE_CAP + 1, cl.LDS_CAP, cl.LDS_CAP + 1} <= {c.H for c in sets["wave"]}
    assert [cl.route_of(c, cl.COMPACT, 0) for c in sets["tandem"]] == ["sketch>wave", "sketch>filter"] * 2 and [c.H for c in sets["tandem"]] == [cl.MID64, cl.MID64 + 1] * 2
    # ---- chunk_finish_kernel: the feature slots on both sides of kRecEntMax
    slots = sorted(len(c.read.feats) for c in sets["chunk"] + sets["chunk15"])
    assert cl.REC_ENT_MAX in slots and cl.REC_ENT_MAX + 1 in slots, slots
    assert {cl.route_of(c, cl.COMPACT, 0) for c in sets["chunk"] + sets["chunk15"]} == {"chunk>filter", "chunk>wave"}
    # ---- 8-byte store
    big = {c.name: c for c in sets["big"]}
    assert (big["big: 64 entries"].entries, big["big: 65 entries"].entries) == (cl.BIG_ENT, cl.BIG_ENT + 1)
    assert [big[f"big: kept {k}"].big_kept() for k in (512, 513, 1024, 1025)] == [(k, k) for k in (512, 513, 1024, 1025)]
    assert [big[f"big: kept {k}, second instance"].big_kept() for k in (512, 513, 1024, 1025)] == [(k, k) for k in (512, 513, 1024, 1025)]
    R = cl.BIG_MAX_ROUNDS
    assert [big[n].big_shape()[:3] for n in ("big: r8 256", "big: r8 257", "big: r16 256", "big: r16 257")] == [(R, R // 2, 3), (R + 1, R // 2 + 1, 4), (2 * R, R, 4), (2 * R + 1, R + 1, 6)]
    assert (big["big: R 256 at 64 lanes"].big_shape()[2:], big["big: R 257 at 64 lanes"].big_shape()[2:]) == ((6, R), (6, R + 1))


def test_strong_and_weak_answers_per_class(sets, capsys):
    """the oracle's answer: K candidates of two or more hits (strong) for some cases of every class, fewer for at least one"""
    count = {}
    for c in everything(sets):
        for store in cl.STORES:
            route = cl.route_of(c, store, cl.case_big_min(c))
            if route == "filter" and store == cl.WIDE8:
                route = "filter>" + cl.big_route(c)
            for K, tax in COMBOS:
                s, w = count.setdefault((store, route), [0, 0])
                count[(store, route)] = [s + c.strong(K, tax), w + (not c.strong(K, tax))]
    with capsys.disabled():
        for k in sorted(count):
            print(f"\n  {k[0]:8} {k[1]:16} strong {count[k][0]:4}  weak {count[k][1]:4}", end="")
        print()
    for k, (s, w) in count.items():
        assert s > 0 and w > 0, (k, s, w)
    want = {"lane", "mid64", "mid128", "mid256", "hash256", "hash512", "hash1024", "wave", "filter", "chunk>filter", "chunk>wave", "sketch>filter", "sketch>wave"}
    assert {r for (st, r) in count if st == cl.COMPACT} == want
    assert {r for (st, r) in count if st == cl.WIDE8} == (want - {"filter", "chunk>filter", "sketch>filter"}) | {"filter>count", "filter>count2", "filter>wave"}


def test_borders_the_lane_path_cannot_reach():
    """each from the constants of the sources"""
    # a lane read: two mates of up to kLaneMaxLen characters, ceil((len - k + 1) / stride) windows each, kLaneS features per window
    wins = len(sketch_ref.windows(cl.LANE_MAX_LEN, cl.KMER, cl.WINLEN, cl.STRIDE))
    most = 2 * wins * cl.LANE_S
    assert (wins, most) == (5, 160)
    assert most < cl.HASH_ENT                                      # hash_cands_kernel's kHashEnt 256 / 257: hashOK never fails on the entries
    assert most < cl.BIG_ENT * cl.BIG_EPL                          # 8-byte store: entries at 192 / 193
    assert most < cl.REC_ENT_MAX                                   # compact store: a lane read's entries always fit the record
    # counting needs maxWin <= kHashWin: both mates together at most (kHashWin - 1) * stride - 1 characters -> 8 windows, 128 entries
    longest = (cl.HASH_WIN - 1) * cl.STRIDE - 1
    a = longest // 2
    ent8 = (len(sketch_ref.windows(a, 16, 127, 112)) + len(sketch_ref.windows(longest - a, 16, 127, 112))) * cl.LANE_S
    assert ent8 == 128
    # big_setup: rounds of 16 or 64 lanes need r8 > kBigMaxRounds; r8 <= (H + 7 * entries) / 8, and a counted list has H <= 1024
    assert (cl.BIG_MAX_FILTERED + 7 * ent8) // 8 < cl.BIG_MAX_ROUNDS + 1
    # ... while the shapes themselves are reachable: 128 entries of 254 locations need 512 rounds of 64 lanes
    assert ent8 * -(-cl.MAX_LIST // 64) > cl.BIG_MAX_ROUNDS
    # chunk_finish_kernel: 4095 slots = 273 windows x 15, 4096 = 256 x 16; no sketch length up to kLaneS has both
    assert [s for s in range(1, cl.LANE_S + 1) if cl.REC_ENT_MAX % s == 0 and (cl.REC_ENT_MAX + 1) % s == 0] == [1]
    # compact store, filter_takes' H <= kMaxHitsPerQuery: a million locations need more feature slots than the record names
    assert cl.REC_ENT_MAX * 255 < cl.MAX_HITS
    # mid_cands_kernel<G>: ceil(n / (256 / G)) blocks of 256 / G groups hold a group for every read of any batch -- no second trip
    for G in (4, 8, 16):
        per_block = 4 * (64 // G)
        assert all(-(-n // per_block) * per_block >= n for n in range(1, 2000)) and per_block == 256 // G
    full = cl.full_list_cases(np.random.default_rng(3))
    assert {k: len(v) for k, v in full.items()} == {"mid64": 65, "mid128": 33, "mid256": 17}
    assert all(cl.route_of(c, st, cl.NO_FILTER) == k for k, v in full.items() for c in v for st in cl.STORES)
    # kLaneK: the lane path takes K <= 4; K = 5 is the wave kernels'
    assert cl.LANE_K == 4
