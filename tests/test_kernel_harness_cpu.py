"""CPU: the kernel harness (tests/cpp/kernel_harness.hip -> libmckharness.so, tests/kernel_harness.py) builds and loads beside the
product library, answers the launchers' host-only size queries, and REFUSES every bad input with its own error code before any device
call -- on a machine without a device a call that got past validation could only answer KH_ERR_HIP.  The numbering helper of the
wrapper against a plain numpy restatement."""
import os

import numpy as np
import pytest

import kernel_harness as kh
from metacache_amd import build


def test_library_is_built_beside_the_product_and_loads():
    L = kh.lib()
    assert os.path.dirname(build.HARNESS_LIB) == os.path.dirname(build.LIB) and os.path.exists(build.HARNESS_LIB)
    for name in ("kh_scan", "kh_order_sort", "kh_sorted_cands", "kh_gw_layout", "kh_constants"):
        assert hasattr(L, name)
    c = kh.constants()
    assert c["kGwMaxKept"] == (1 << 20) - 1 and c["kGwGap"] == 1024 and c["kFlagDone"] == 0 and c["kFlagCands"] == 2
    assert c["kCntSorted"] == 13 and c["kCntSortedBig"] == 18 and c["kCntSortedBig"] < c["kCounterWords"]
    # the constants the GPU tests read from the kernel files
    assert kh.source_constant("kernels.hip", "kScanTile") == 2048 and kh.source_constant("kernels.hip", "kSmallScan") == 16384
    assert kh.source_constant("gw_kernels.hip", "kGwFewBig") == 1024 and kh.source_constant("gw_kernels.hip", "kGwBigSorted") == 8192


def test_size_queries_grow_with_their_arguments():
    L = kh.lib()
    tile = kh.source_constant("kernels.hip", "kScanTile")
    scan = [L.kh_scan_tmp_bytes(n) for n in (0, 1, tile, tile + 1, 16 * tile, 1 << 20, (1 << 20) + 1)]
    assert scan[0] >= 16 and all(b >= a for a, b in zip(scan, scan[1:])) and scan[3] > scan[2] and scan[6] > scan[5] > scan[4]
    # one block sum per tile, the grand total behind them
    assert all(L.kh_scan_tmp_bytes(n) >= ((n + tile - 1) // tile + 1) * 8 for n in (1, tile, tile + 1, 1 << 20))
    # the order's scratch is `count` words + this: it must hold one cursor per length class and never shrink
    order = [L.kh_order_temp_bytes(n, c) for n, c in ((1, 1), (5000, 100), (5000, 5000), (1 << 20, 1 << 20))]
    assert order[0] >= 4097 * 4 and all(b >= a for a, b in zip(order, order[1:]))
    # the sort's temp: plan words per list + the scan's block sums + a second pool for the merge passes
    seg = {(s, p): L.kh_segsort_temp_bytes(max(s, 1), s, p) for s in (1, 1000, 100000) for p in (1, 1 << 16, 1 << 24)}
    for s in (1, 1000, 100000):
        assert seg[(s, 1)] < seg[(s, 1 << 16)] < seg[(s, 1 << 24)] and seg[(s, 1 << 24)] >= (1 << 24) * 4
    for p in (1, 1 << 16, 1 << 24):
        assert seg[(1, p)] < seg[(1000, p)] < seg[(100000, p)] and seg[(100000, p)] - seg[(1, p)] >= 4 * 4 * 99999


def numpy_layout(windows, gap):
    windows = np.asarray(windows, dtype=np.int64)
    base = gap + np.concatenate(([0], np.cumsum(windows + gap)))
    total = int(base[-1])
    shift = 6
    while (total >> shift) + 2 > (1 << 22):
        shift += 1
    blocks = np.arange((total >> shift) + 2, dtype=np.int64) << shift
    # the target whose numbers, the gap behind them included, hold max(block, gap); the last target takes what lies behind it
    d = np.minimum(np.searchsorted(base, np.maximum(blocks, gap), side="right") - 1, len(windows) - 1)
    return base, shift, d


@pytest.mark.parametrize("windows,gap", [
    ([1], 8), ([5, 1, 1, 700, 3], 1024), ([1] * 300, 8), ([40000, 1, 90000, 17, 64, 63, 65], 1024),
    (np.random.default_rng(5).integers(1, 3000, 2000), 1024), ([60_000_000] * 6, 1024)])
def test_numbering_helper_and_directory_against_numpy(windows, gap):
    lay = kh.GwLayout(windows, gap)
    base, shift, d = numpy_layout(windows, gap)
    assert np.array_equal(lay.base.astype(np.int64), base) and lay.shift == shift and np.array_equal(lay.dir.astype(np.int64), d)
    if len(windows) == 6:
        assert shift > 6                                           # (the directory is capped at 2^22 entries)
    rng = np.random.default_rng(len(windows))
    w = np.asarray(windows, dtype=np.int64)
    tgt = np.concatenate((rng.integers(0, len(w), 500), [0, len(w) - 1, 0, len(w) - 1]))
    win = np.concatenate((rng.integers(0, 1 << 62, 500) % w[tgt[:500]], [0, 0, w[0] - 1, w[-1] - 1]))
    gw = lay.numbers(tgt, win)
    assert np.array_equal(gw.astype(np.int64), base[tgt] + win)
    t2, w2 = lay.split(gw)
    assert np.array_equal(t2, tgt) and np.array_equal(w2, win)
    assert np.array_equal(lay.locations(gw), (tgt.astype(np.uint64) << np.uint64(32)) | win.astype(np.uint64))
    # a searched-for target is the directory's entry advanced by at most the targets that begin inside one block
    per_block = np.bincount((base[1:-1] >> shift), minlength=len(d)) if len(w) > 1 else np.zeros(len(d), np.int64)
    blk = gw.astype(np.int64) >> shift
    ahead = tgt - lay.dir[blk].astype(np.int64)
    assert np.all(ahead >= 0) and np.all(ahead <= per_block[blk])


def test_layouts_that_cannot_be_numbered_are_refused():
    for windows, gap in (([], 1024), ([5], 7), ([0xFFFFFFF0], 1024), ([1 << 31, 1 << 31], 1024)):
        with pytest.raises(kh.HarnessError) as e:
            kh.GwLayout(windows, gap)
        assert e.value.code == kh.ERR_TABLE


def refused(call, *a, **kw):
    with pytest.raises(kh.HarnessError) as e:
        call(*a, **kw)
    return e.value.code


def test_scan_refuses_bad_arguments():
    v = np.arange(10, dtype=np.uint32)
    assert refused(kh.scan, v, stride=0, n=5) == kh.ERR_ARG
    assert refused(kh.scan, v, want32=False, want64=False) == kh.ERR_ARG
    assert refused(kh.scan, v, stride=1 << 20, n=1 << 20) == kh.ERR_ARG


M = (1 << 20) - 1        # kGwMaxKept


def test_order_sort_refuses_each_bad_input():
    pool = np.arange(100, dtype=np.uint32)
    ok = dict(n=4, lengths=[10, 20], offsets=[0, 10], pool=pool)
    bad = lambda **kw: refused(kh.order_sort, **{**ok, **kw})      # noqa: E731
    assert bad(n=0) == kh.ERR_ARG
    assert bad(lengths=[], offsets=[]) == kh.ERR_COUNT
    assert bad(n=1) == kh.ERR_COUNT                                # nlists > n
    assert bad(lengths=[10, 0]) == kh.ERR_LENGTH
    assert bad(lengths=[10, M + 1], pool=np.zeros(M + 20, np.uint32)) == kh.ERR_LENGTH
    assert bad(offsets=[0, 81]) == kh.ERR_RANGE                    # 81 + 20 > 100
    assert bad(offsets=[0, 0xFFFFFFFF]) == kh.ERR_RANGE            # (no 32-bit wrap)
    assert bad(offsets=[0, 9]) == kh.ERR_OVERLAP
    assert bad(offsets=[15, 0]) == kh.ERR_OVERLAP                  # [15, 25) and [0, 20)
    p = pool.copy(); p[29] = 0xFFFFFFFF
    assert bad(pool=p) == kh.ERR_PADDING
    # ... and what is legal gets past validation: without a device the first device call fails, with one the call succeeds
    p = pool.copy(); p[30] = 0xFFFFFFFF                            # outside every list: the sentinel of the GPU tests
    assert passes_validation(kh.order_sort, **{**ok, "pool": p})
    assert passes_validation(kh.order_sort, **{**ok, "lengths": [10, M], "pool": np.zeros(M + 10, np.uint32)})
    assert passes_validation(kh.order_sort, **{**ok, "n": 2, "offsets": [80, 0]})


def passes_validation(call, *a, **kw):
    try:
        call(*a, **kw)
    except kh.HarnessError as e:
        return e.code == kh.ERR_HIP
    return True


def test_sorted_cands_refuses_each_bad_input():
    lay = kh.GwLayout([50, 1, 30], 16)                             # base 16, 82, 99, 145: windows [16, 66), [82, 83), [99, 129)
    assert list(lay.base) == [16, 82, 99, 145]
    a = lay.numbers([0, 0, 1, 2, 2], [0, 49, 0, 0, 29])
    b = lay.numbers([0, 2], [7, 7])
    lengths, offsets, pool = kh.pack_lists([a, b])
    ok = dict(n=3, lengths=lengths, offsets=offsets, pool=pool, max_win=[2, 16], q=[2, 0], qhits=[5, 2], layout=lay, K=2, taxkey=None)
    bad = lambda **kw: refused(kh.sorted_cands, **{**ok, **kw})    # noqa: E731

    def with_number(i, v):
        p = pool.copy(); p[i] = v
        return p
    # what the order/sort entry checks holds here too
    assert bad(n=1) == kh.ERR_COUNT
    assert bad(lengths=[5, 0]) == kh.ERR_LENGTH
    assert bad(offsets=[0, 6]) == kh.ERR_RANGE
    assert bad(offsets=[0, 4]) == kh.ERR_OVERLAP
    assert bad(pool=with_number(1, 0xFFFFFFFF)) == kh.ERR_PADDING
    # numbers outside every target's windows: before the first target, in a gap (both ends), behind the last target, beyond gwBase[targets]
    for i, v in ((0, 15), (0, 0), (1, 66), (1, 81), (2, 83), (4, 129), (4, 144), (4, 145), (4, 0xFFFFFFFE)):
        assert bad(pool=with_number(i, v)) == kh.ERR_WINDOW, (i, v)
    assert bad(pool=with_number(2, 60)) == kh.ERR_ORDER            # 16, 65, 60: a window of target 0, but behind a larger number
    assert bad(pool=with_number(6, 20)) == kh.ERR_ORDER            # the second list: 23, 20
    assert bad(max_win=[0, 16]) == kh.ERR_MAXWIN
    assert bad(max_win=[2, 17]) == kh.ERR_MAXWIN                   # beyond the gap
    assert bad(K=0) == kh.ERR_K
    assert bad(K=5) == kh.ERR_K
    assert bad(q=[2, 3]) == kh.ERR_QUERY                           # q >= n
    assert bad(q=[1, 1]) == kh.ERR_QUERY                           # the same read twice
    assert bad(layout=_raw_layout([50, 1, 30], 7)) == kh.ERR_TABLE
    assert bad(layout=_raw_layout([], 16)) == kh.ERR_TABLE
    # legal: equal neighbours, the widest window range, every K, a taxon map
    assert passes_validation(kh.sorted_cands, **{**ok, "pool": with_number(1, 16)})
    assert passes_validation(kh.sorted_cands, **{**ok, "max_win": [16, 1], "K": 4, "taxkey": [1, 0, 1]})


class _raw_layout:
    """a layout the wrapper would refuse to build, handed to the library as it is"""

    def __init__(self, windows, gap):
        self.windows, self.gap = np.asarray(windows, dtype=np.uint32), gap
