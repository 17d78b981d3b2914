"""CPU: the inputs of tests/test_gpu_owner_filtered_path.py are proved here, before any kernel sees them -- every border case has the
shape and the route it was named for and is kept whole by the filters (kept_lo == kept_hi), the oracle's answer is what the case was
built for, every route of owner_lists.ROUTES is reached, the packing reads back, and the pool cases do cross the rules of
owner_numbers_pool / big_filter_grid."""
import numpy as np
import pytest

import owner_lists as ol

FUSES = (1, 6, 5, 0)


@pytest.fixture(scope="module")
def sets():
    rng = np.random.default_rng(2025)
    return dict(border=ol.border_cases(rng), ties=ol.tie_cases(rng) + [ol.two_regions_case(rng)], weak=ol.weak_cases(rng), many=ol.too_many_case(rng))


def test_table_numbering():
    assert ol.GAP == 1024 and ol.BASE[0] == ol.GAP and np.all(np.diff(ol.BASE) == ol.WINDOWS.astype(np.int64) + ol.GAP)
    assert ol.WINDOWS[0] == 1 and ol.WINDOWS[ol.WIDE[0]] == 6000 and ol.WINDOWS.min() == 1 and ol.WINDOWS.max() == 6000
    assert (ol.TAX == 0).sum() > 20 and np.all(ol.TAX[0:3] == 1)
    t, w = ol.split(ol.numbers([0, 5, ol.NT - 1], [0, 7, 3]))
    assert t.tolist() == [0, 5, ol.NT - 1] and w.tolist() == [0, 7, 3]
    tt, _ = ol.split(np.concatenate((ol.TRAP, ol.TRAP_SLACK)))
    assert np.all(tt == ol.TRAP_T)


def test_border_cases_have_the_shape_and_route_they_were_named_for(sets):
    names = set()
    for c in sets["border"]:
        assert c.name not in names, c.name
        names.add(c.name)
        assert c.kept_lo == c.kept_hi == c.H == c.named["H"], (c.name, c.kept_lo, c.H)
        assert c.rounds == c.named["rounds"], (c.name, c.rounds)
        if "distinct" in c.named:
            assert c.distinct == c.distinct_hi == c.named["distinct"], (c.name, c.distinct)
        assert ol.route_of(c, **c.named["tuning"]) == c.named["route"] and c.named["route"] in ol.ROUTES, (c.name, ol.route_of(c, **c.named["tuning"]))
    by = {c.name: c for c in sets["border"]}
    # the borders from both sides, as numbers
    assert (by["H 64"].H, by["H 65"].H) == (ol.MID64, ol.MID64 + 1)
    assert [len(p) for p in by["pieces of 0 1 2 15 16 17 30"].pieces] == [0, 1, 2, 15, 16, 17, 30]
    assert len(by["piece of 65 535"].pieces[0]) == ol.PIECE_MAX and by["piece of 65 535"].takes() and not by["piece of 65 536"].takes()
    assert not by["piece of 65 536 beside short ones"].takes() and by["piece of 65 536 beside short ones"].H > ol.MID64
    assert by["16 pieces of 65 535"].H <= ol.MAX_HITS < sets["many"].H and ol.route_of(sets["many"]) == "too_many"
    assert {c.S for c in sets["border"]} >= {1, 2, 3, 63, 64}
    assert (by["H 2 048 in 128 rounds"].H, by["H 2 048 in 128 rounds"].rounds) == (ol.SMALL_H, ol.ROUNDS)
    assert (by["H 2 049 in 128 rounds"].H, by["H 2 049 in 128 rounds"].rounds) == (ol.SMALL_H + 1, ol.ROUNDS)
    assert (by["128 rounds"].rounds, by["129 rounds"].rounds) == (ol.ROUNDS, ol.ROUNDS + 1) and by["129 rounds"].H <= ol.SMALL_H
    assert (by["256 rounds"].rounds, by["257 rounds"].rounds) == (ol.F2_ROUNDS, ol.F2_ROUNDS + 1) and by["257 rounds"].H <= ol.F2_H
    assert (by["H 4 096 in 256 rounds"].H, by["H 4 097 in 256 rounds"].H) == (ol.F2_H, ol.F2_H + 1)
    assert by["H 4 096 in 256 rounds"].rounds == by["H 4 097 in 256 rounds"].rounds == ol.F2_ROUNDS
    assert (by["maxWin 8"].max_win, by["maxWin 9"].max_win, by["maxWin 1 024"].max_win, by["maxWin 1 025"].max_win) == (ol.HASH_WIN, ol.HASH_WIN + 1, ol.GAP, ol.GAP + 1)
    assert (by["H 32 768"].H, by["H 32 769"].H) == (ol.BIG_H, ol.BIG_H + 1)
    assert (by["H 8 192, gw_mid_h 8 192"].H, by["H 8 193, gw_mid_h 8 192"].H) == (ol.BIG_SORTED, ol.BIG_SORTED + 1)
    for k in (256, 257, 384, 385, 512, 513, 1024, 1025):
        assert by[f"kept {k}"].kept_lo == k and by[f"kept {k}"].distinct <= ol.FUSED_DISTINCT
    assert (by["kept 384, 256 distinct"].distinct, by["kept 384, 257 distinct"].distinct) == (ol.FUSED_DISTINCT, ol.FUSED_DISTINCT + 1)
    # the other instances of the fused kernel, and the two kernels apart
    want = {"kept 256": {6: "fused", 5: "fused", 0: "filter>count9"}, "kept 257": {6: "fused", 5: "fused", 0: "filter>count10"},
            "kept 384": {6: "fused", 5: "fused", 0: "filter>count10"}, "kept 385": {6: "filter>count10", 5: "fused", 0: "filter>count10"},
            "kept 512": {6: "filter>count10", 5: "fused", 0: "filter>count10"}, "kept 513": {6: "filter>count11", 5: "filter>count11", 0: "filter>count11"},
            "kept 384, 257 distinct": {6: "filter>count10", 5: "filter>count10", 0: "filter>count10"},
            "H 65": {6: "fused", 5: "fused", 0: "filter>count9"}, "maxWin 9": {6: "filter>sorted_wave", 5: "filter>sorted_wave", 0: "filter>sorted_wave"}}
    for name, routes in want.items():
        for fuse, r in routes.items():
            assert ol.route_of(by[name], fuse=fuse) == r, (name, fuse, ol.route_of(by[name], fuse=fuse))
    # "gw_big_h" 0 and 2 048: every read past gw_filter2 takes one instance of the stream filter, then the other
    for c in sets["border"]:
        r0, r1 = ol.route_of(c, big_h=0), ol.route_of(c, big_h=2048)
        if r0.startswith("stream"):
            assert r0.startswith("stream>") and r1.startswith("stream_fine>"), (c.name, r0, r1)
    # the border call's pool slices have the room the routes assume, with every tuning the GPU test runs it with
    n = len(sets["border"]) + 9
    for fuse in FUSES:
        for kw in (dict(), dict(mid_h=8192), dict(big_h=2048), dict(big_h=0)):
            assert ol.filter2_room(sets["border"], n, fuse=fuse, **kw), (fuse, kw)


def test_the_oracle_answers_what_the_cases_were_built_for(sets):
    for c in sets["border"] + sets["ties"]:
        for K, lowest in ol.COMBOS:
            assert c.strong(K, lowest != 0), (c.name, K, lowest, c.expected(K, lowest != 0))
    for c in sets["weak"]:
        for K, lowest in ol.COMBOS:
            tax = lowest != 0
            weak = K >= c.named["weak_from"] and (tax or not c.named.get("weak_tax_only"))
            assert c.strong(K, tax) == (not weak), (c.name, K, lowest, c.expected(K, tax))
        assert ol.route_of(c, **c.named["tuning"]) == c.named["route"], (c.name, ol.route_of(c, **c.named["tuning"]))
    assert sets["many"].expected(1, False) is None
    # the tie rules: what the oracle says about them
    by = {c.name: c for c in sets["ties"]}
    e = by["equal hits across nine targets"].expected(4, False)
    assert e["tgt"].tolist() == [200, 201, 202, 203] and e["hits"].tolist() == [3, 3, 3, 3]            # the lower target wins
    e = by["equal hits twice in one target, 3 between"].expected(2, False)
    assert (int(e["tgt"][0]), int(e["hits"][0]), int(e["beg"][0]), int(e["end"][0])) == (ol.WIDE[11], 4, 10, 13)   # the first of two equal ranges
    e = by["later range with more hits"].expected(1, False)
    assert (int(e["tgt"][0]), int(e["hits"][0]), int(e["beg"][0])) == (ol.WIDE[13], 5, 3000)
    e = by["first and last target, one-window targets"].expected(4, False)
    assert e["tgt"].tolist()[:2] == [ol.ONEWIN[1], ol.NT - 1] or e["hits"].tolist()[0] == 5
    # two regions of one target with the most hits: the counting without taxon merging picks both and hands the read back
    c = by["two regions of one target lead"]
    assert ol.handed_back(c, "fused", 2, False) is True and ol.handed_back(c, "fused", 1, False) is False and ol.handed_back(c, "fused", 2, True) is False
    assert ol.handed_back(by["equal hits across nine targets"], "fused", 4, False) is False


def test_every_route_is_reached_by_a_strong_and_a_weak_case(sets, capsys):
    reached = {r: [0, 0] for r in ol.ROUTES}
    cases = sets["border"] + sets["ties"] + sets["weak"] + [sets["many"], ol.Case("no numbers", [np.zeros(0, np.uint32)] * 3, 4)]
    for c in cases:
        own = c.named.get("tuning", {})
        for fuse in FUSES:
            r = ol.route_of(c, **dict(own, fuse=fuse))
            assert r in ol.ROUTES, (c.name, fuse, r)
            if fuse != 1 and r == ol.route_of(c, **own):
                continue                                            # (counted once unless the instance changes the route)
            strong = any(c.strong(K, lowest != 0) for K, lowest in ol.COMBOS)
            weak = any(c.expected(K, lowest != 0) is not None and not c.strong(K, lowest != 0) for K, lowest in ol.COMBOS)
            reached[r][0] += strong
            reached[r][1] += weak
    with capsys.disabled():
        print("\nroute: strong cases, weak cases")
        for r, (s, w) in reached.items():
            print(f"  {r:26s} {s:3d} {w:3d}")
    for r, back in ol.ROUTES.items():
        if r in ("empty", "too_many"):
            continue
        assert reached[r][0] >= 1, (r, reached[r])
        assert reached[r][1] >= 1 or not back, (r, reached[r])


def test_packing_reads_back(sets):
    rng = np.random.default_rng(5)
    cases = sets["border"] + sets["weak"]
    for n, S in ((len(cases), None), (len(cases) + 300, 64)):
        at = rng.permutation(n)[:len(cases)]
        counts, nums, offsets, max_win = ol.pack(cases, at, n, S)
        S_call = len(offsets) - 1
        assert S_call == 64 and len(counts) == S_call * n and int(offsets[-1]) == len(nums) == sum(c.H for c in cases)
        back = ol.unpack(counts, nums, offsets, n)
        for c, q in zip(cases, at):
            assert max_win[q] == c.max_win
            for s in range(S_call):
                want = c.pieces[s] if s < c.S else np.zeros(0, np.uint32)
                assert np.array_equal(back[q][s], want), (c.name, s)
        rest = np.setdiff1d(np.arange(n), at)
        assert all(len(p) == 0 for q in rest for p in back[q])
        # pieces begin at every offset 0 .. 3 mod 4 words of the buffer
        cm = counts.reshape(S_call, n).astype(np.int64)
        begin = (offsets[:-1].astype(np.int64)[:, None] + np.cumsum(cm, axis=1) - cm)[cm > 0]
        assert set((begin % 4).tolist()) == {0, 1, 2, 3}


def test_pool_cases_cross_the_rules():
    rng = np.random.default_rng(6)
    # one read of 10^5 kept numbers among short ones: no slice can take it, the overflow region can
    cases, at, n = ol.overflow_batch(rng)
    total = sum(c.H for c in cases)
    slices, cap, ovf = ol.pool_sizes(n, total)
    big = max(c.H for c in cases)
    assert big == 100_000 and cap < big <= ovf and total < 2_100_000 and slices == 4 * ((n + 3) // 4), (slices, cap, ovf)
    assert ol.route_of(cases[3]) == "stream_fine>sorted_block" and cases[3].kept_lo == big
    counts, nums, offsets, _ = ol.pack(cases, at, n)
    assert len(nums) == total and at[0] == 0 and at[-1] == n - 1 and np.count_nonzero(counts.reshape(-1, n).sum(axis=0)) == len(cases)
    # "filter_bpc" 1: 1 024 waves walk five and more reads each; the slice of a wave is full after five
    cases, at, n = ol.full_slices_batch(rng)
    total = sum(c.H for c in cases)
    slices, cap, ovf = ol.pool_sizes(n, total, filter_bpc=1)
    kept = cases[0].kept_lo
    assert all(c.kept_lo == c.kept_hi == kept and c.H <= ol.SMALL_H and c.rounds <= ol.ROUNDS and c.takes() for c in cases[:8])
    assert all(ol.route_of(c) in ("filter>count10", "filter>sorted_wave") for c in cases[:8])      # every list goes through the pool
    assert slices == 1024 and n > 5 * slices and total <= 2_300_000
    assert cap - 4 * kept >= ol.SLICE_RESERVE > cap - 5 * kept, (cap, kept)                        # the sixth read of a wave is sent on
    assert cap - 5 * kept >= kept                                                                  # ... and a slice of its block still takes its list
