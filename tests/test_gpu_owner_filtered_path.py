"""GPU: the compact store's filtered path -- gw_filter_count_kernel / gw_filter_kernel, gw_filter2_kernel, gw_compact_kernel, the three
gw_filter_stream_kernel instances, gw_count_kernel<9 / 10 / 11>, the sorted tail -- and the owner side of Mode K in front of it
(owner_entries_kernel, decode_union_kernel, the per-source scans) at their borders, through ONE public call:
mc_candidates_from_partial_numbers takes the numbers themselves, so a list is put exactly on a border (tests/owner_lists.py; the
inputs are proved in tests/test_owner_lists_cpu.py).  Whatever route a read takes, its candidates must be the oracle's
candidates_from_list on the sorted union of the same locations: exact integer equality, plus the statistics words, mc_owner_stats and
the sorted tail's timers against the model.  One context per max_candidates (it is part of the configuration), made once per module."""
import ctypes as C

import numpy as np
import pytest

import owner_lists as ol

pytestmark = pytest.mark.gpu

FUSES = (1, 6, 5, 0)                  # "gw_fuse": the seven- (default), six- and five-wave instances of the fused kernel, the two kernels apart


@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(2025)
    w = dict(border=ol.border_cases(rng), ties=ol.tie_cases(rng) + [ol.two_regions_case(rng)], weak=ol.weak_cases(rng), many=ol.too_many_case(rng), db={})

    def db(K):
        if K not in w["db"]:
            w["db"][K] = ol.context(K)
        return w["db"][K]
    w["ctx"] = db
    yield w
    for d in w["db"].values():
        d.close()


def _spread(rng, k, n):
    """k reads of a batch of n: the first, the last, the others anywhere"""
    at = [0, n - 1][:min(k, n)] if n > 1 else [0]
    rest = [q for q in rng.permutation(n).tolist() if q not in at]
    return at + rest[:k - len(at)]


@pytest.mark.parametrize("K,lowest", ol.COMBOS)
def test_borders_against_the_oracle(world, K, lowest):
    """every border of tests/owner_lists.border_cases from both sides, the tie rules, and the weak reads beside the one read that has
    more locations than a read may have -- with every instance of the first kernel"""
    rng = np.random.default_rng(10 * K + lowest)
    db = world["ctx"](K)
    strong = world["border"] + world["ties"]
    weak = world["weak"] + [world["many"]]
    reached = {}
    for fuse in FUSES:
        for cases, extra in ((strong, 9), (weak, 4)):
            n = len(cases) + extra
            assert ol.filter2_room(cases, n, fuse=fuse)
            r = ol.check(db, cases, K, lowest, n=n, order=_spread(rng, len(cases), n), fuse=fuse, shift=fuse % 4)
            for k, v in r.items():
                reached[k] = reached.get(k, 0) + v
    assert set(reached) == set(ol.ROUTES) - {"empty", "stream_mid>sorted_wave", "stream_fine>sorted_wave"}, sorted(set(ol.ROUTES) - set(reached))


@pytest.mark.parametrize("K,lowest", [(2, 0), (4, ol.TAX_RANK)])
@pytest.mark.parametrize("tuning", [dict(mid_h=8192), dict(big_h=2048), dict(big_h=0)], ids=["mid_h 8192", "big_h 2048", "big_h 0"])
def test_stream_filter_instances(world, tuning, K, lowest):
    """"gw_mid_h" 8 192: H = 8 192 / 8 193 on both sides of the small-filter instance; "gw_big_h" 0 and 2 048: every read past gw_filter2
    takes the default instance, then the fine-block one"""
    rng = np.random.default_rng(77 + K)
    db = world["ctx"](K)
    reached = {}
    for cases, extra in ((world["border"], 9), (world["weak"] + [world["many"]], 4)):
        n = len(cases) + extra
        r = ol.check(db, cases, K, lowest, n=n, order=_spread(rng, len(cases), n), **tuning)
        for k, v in r.items():
            reached[k] = reached.get(k, 0) + v
    streams = {k.split(">")[0] for k in reached if k.startswith("stream")}
    want = {"mid_h": {"stream", "stream_mid", "stream_fine"}, "big_h": {"stream_fine"} if tuning.get("big_h") else {"stream"}}["mid_h" if "mid_h" in tuning else "big_h"]
    assert streams == want, reached


@pytest.mark.parametrize("S", [1, 2, 3, 63, 64])
def test_source_counts_and_piece_offsets(world, S):
    """S sources (reads with fewer pieces have empty ones), the payload at every offset 0 .. 3 words behind a 16-byte border"""
    rng = np.random.default_rng(S)
    db = world["ctx"](2)
    cases = [c for c in world["border"] + world["ties"] + world["weak"] if c.S <= S and c.H <= 70_000 and "filter2" not in ol.route_of(c)]
    assert len(cases) >= 6 and any(c.S == S for c in cases)
    for shift in range(4):
        n = len(cases) + 3
        ol.check(db, cases, 2, ol.TAX_RANK if shift % 2 else 0, n=n, order=_spread(rng, len(cases), n), S=S, shift=shift)


def test_no_source_and_too_many_sources_are_refused(world):
    import torch
    from metacache_amd import api
    db = world["ctx"](2)
    dev = torch.device("cuda", 0)
    n = 4
    counts = torch.zeros(65 * n, dtype=torch.int32, device=dev)
    nums = torch.from_numpy(np.tile(ol.TRAP, 8).view(np.int32)).to(dev)
    mw = torch.full((n,), 3, dtype=torch.int32, device=dev)
    L = api.lib()
    for S in (0, 65):
        so = np.zeros(S + 1, dtype=np.uint64)
        h = api.McDevicePartialNumbersIn(counts.data_ptr(), nums.data_ptr(), so.ctypes.data, mw.data_ptr(), 0, n, S)
        r = api.McDeviceResults()
        L.mc_candidates_from_partial_numbers.argtypes = [C.c_void_p, C.POINTER(api.McDevicePartialNumbersIn), C.c_int, C.POINTER(api.McDeviceResults), C.c_void_p]
        assert L.mc_candidates_from_partial_numbers(db.h, C.byref(h), 0, C.byref(r), None) == ol.MC_ERR_INVALID, S
    before = ol.owner_stats(db)
    res = db.candidates_from_partial_numbers(counts.data_ptr(), nums.data_ptr(), np.zeros(65, np.uint64), n, max_win_ptr=mw.data_ptr())   # 64: taken
    db.synchronize()
    assert res.cands and (ol.owner_stats(db) - before).tolist() == [n, 0, 0, 0]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 3000])
def test_batch_shapes(world, n):
    """cases at the first and the last read, the other reads without numbers; the same cases in two orders"""
    rng = np.random.default_rng(n)
    db = world["ctx"](2)
    by = {c.name: c for c in world["border"] + world["weak"] + world["ties"]}
    names = ["kept 385", "maxWin 9", "pieces of 4 000", "H 64", "one strong target and 40 single hits", "kept 1025", "equal hits across nine targets",
             "kept 256", "single hits only", "257 rounds"]
    cases = [by[k] for k in names][:n]
    at = _spread(rng, len(cases), n)
    for K, lowest in ((2, 0), (2, ol.TAX_RANK)):
        ol.check(db, cases, K, lowest, n=n, order=at)
        ol.check(db, cases, K, lowest, n=n, order=at[::-1])


def test_a_list_no_slice_can_take_goes_to_the_overflow_region(world):
    rng = np.random.default_rng(6)
    cases, at, n = ol.overflow_batch(rng)
    slices, cap, ovf = ol.pool_sizes(n, sum(c.H for c in cases))
    assert cap < max(c.H for c in cases) <= ovf
    for K, lowest in ((2, 0), (4, ol.TAX_RANK)):
        ol.check(world["ctx"](K), cases, K, lowest, n=n, order=at)


def test_full_pool_slices_send_later_reads_on(world):
    """"filter_bpc" 1: a wave walks five and more reads, the sixth finds less room in its slice than a batch may keep and is left to the
    stream filter (tests/test_owner_lists_cpu.py asserts that the sizes cross the rule)"""
    rng = np.random.default_rng(6)
    cases, at, n = ol.full_slices_batch(rng)
    r = ol.check(world["ctx"](2), cases, 2, 0, n=n, order=at, filter_bpc=1, pool_may_hand_back=True)
    assert sum(r.values()) == n
