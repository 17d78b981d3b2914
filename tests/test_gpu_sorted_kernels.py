"""GPU: the three device stages behind long reads -- launch_scan_u32, launch_gw_order + launch_gw_segsort (gw_sort.hip) and
gw_sorted_cands_kernel (gw_kernels.hip) -- driven DIRECTLY through the kernel harness (tests/cpp/kernel_harness.hip) with inputs built
for the kernels' instance borders, not with whatever lists reads happen to produce.  Models: numpy.cumsum in uint64, numpy.sort per
list, and the oracle's candidates_from_list (cpuref.oracle().candidates, the function mco_query itself uses).  Every comparison is
exact integer equality."""
import numpy as np
import pytest

import cpuref
import kernel_harness as kh

pytestmark = pytest.mark.gpu

C = kh.constants()
MAX_KEPT = C["kGwMaxKept"]
SCAN_TILE = kh.source_constant("kernels.hip", "kScanTile")
SMALL_SCAN = kh.source_constant("kernels.hip", "kSmallScan")
FEW_BIG = kh.source_constant("gw_kernels.hip", "kGwFewBig")
BIG_SORTED = kh.source_constant("gw_kernels.hip", "kGwBigSorted")
WHOLE_MAX, CHUNK, TILE = (kh.source_constant("gw_sort.hip", k) for k in ("kWholeMax", "kChunk", "kTile"))


# ======================================================================================================================
# launch_scan_u32 against numpy.cumsum in uint64
# ======================================================================================================================
SCAN_N = sorted({0, 1, 255, 256, 257, 4095, 4096, 4097, SMALL_SCAN - 1, SMALL_SCAN, SMALL_SCAN + 1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1,
                 3 * SCAN_TILE - 1, 3 * SCAN_TILE, 3 * SCAN_TILE + 1, 9 * SCAN_TILE - 1, 9 * SCAN_TILE, 9 * SCAN_TILE + 1,
                 257 * SCAN_TILE - 1, 257 * SCAN_TILE, 257 * SCAN_TILE + 1, (1 << 20) + 1})


@pytest.mark.parametrize("stride", [1, 4])
@pytest.mark.parametrize("values", ["zero", "max", "random"])
def test_scan_against_cumsum(values, stride):
    assert SMALL_SCAN == 16384 and SMALL_SCAN + 1 in SCAN_N        # the border between the one-block kernel and the three-kernel path
    rng = np.random.default_rng(stride * 7 + len(values))
    bad = []
    for n in SCAN_N:
        src = rng.integers(0, 1 << 32, max(n * stride, 1), dtype=np.uint64).astype(np.uint32)   # (stride 4: three other words between two elements)
        v = {"zero": np.zeros(n, np.uint32), "max": np.full(n, 0xFFFFFFFF, np.uint32), "random": src[:n * stride:stride].copy()}[values]
        src[:n * stride:stride] = v
        ref = np.concatenate(([0], np.cumsum(v.astype(np.uint64), dtype=np.uint64))).astype(np.uint64)
        if values == "max" and n > 1:
            assert int(ref[-1]) >= 1 << 32 or n < 2                # the 64-bit result passes 2^32
        for want32, want64 in ((True, False), (False, True), (True, True)):
            o32, o64, total = kh.scan(src, stride, n, want32, want64, True)
            if want32 and not np.array_equal(o32, (ref & np.uint64(0xFFFFFFFF)).astype(np.uint32)):
                bad.append((n, want32, want64, "out32", int(np.flatnonzero(o32 != (ref & np.uint64(0xFFFFFFFF)).astype(np.uint32))[0])))
            if want64 and not np.array_equal(o64, ref):
                bad.append((n, want32, want64, "out64", int(np.flatnonzero(o64 != ref)[0])))
            if total != int(ref[-1]):
                bad.append((n, want32, want64, "host total", total, int(ref[-1])))
    assert not bad, bad[:10]


def test_scan_without_host_total_leaves_it_alone():
    v = np.arange(40000, dtype=np.uint32)
    for n in (100, 40000):
        o32, o64, total = kh.scan(v, 1, n, True, True, False)
        assert total is None and int(o64[n]) == n * (n - 1) // 2 and int(o32[n]) == (n * (n - 1) // 2) & 0xFFFFFFFF


# ======================================================================================================================
# launch_gw_order + launch_gw_segsort against numpy.sort per list
# ======================================================================================================================
SENTINEL = 0x80000001            # pool words outside every list (a legal number: a kernel that reads or writes one too far shows)
BORDER_LENGTHS = [1, 2, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385, 20480, 20481,
                  32767, 32768, 32769, 49152, 49153, 65536, 65537, 5 * 16384 + 7, 131073, 262145, 524289, MAX_KEPT]


def merge_passes(length: int) -> int:
    p, run = 0, CHUNK
    while run < length:
        p, run = p + 1, run * 2
    return p


def random_numbers(rng, length):
    return rng.integers(0, 0xFFFFFFFF, length, dtype=np.uint64).astype(np.uint32)      # below 2^32 - 1: 0xFFFFFFFE is the largest key


def check_order_sort(lists, n, second, rng, shuffle=True):
    if shuffle:
        lists = [lists[i] for i in rng.permutation(len(lists))]
    lengths, offsets, pool = kh.pack_lists(lists, SENTINEL, rng=rng)
    side, out, after = kh.order_sort(n, lengths, offsets, pool, second_stream=second)
    expected = pool.copy()
    for off, x in zip(offsets.astype(np.int64), lists):
        expected[off:off + len(x)] = np.sort(x)
    if not np.array_equal(out, expected):                          # every list sorted, every word outside the lists as it was
        first = int(np.flatnonzero(out != expected)[0])
        i = int(np.searchsorted(offsets.astype(np.int64), first, side="right") - 1)
        inside = first < int(offsets[i]) + int(lengths[i])
        raise AssertionError(f"sorted pool differs at word {first}: " + (f"list {i} of {int(lengths[i])} numbers, place {first - int(offsets[i])}"
                             if inside else f"a sentinel word behind list {i}") + f" (n {n}, {len(lists)} lists, second stream {second})")
    assert np.array_equal(after, pool), "the sort wrote into its input"
    assert np.array_equal(np.sort(side), np.arange(len(lists))), "the ordered side list is no permutation of the input"
    cls = (lengths[side].astype(np.int64) - 1) >> 8
    assert np.all(cls[1:] <= cls[:-1]), "the side list is not longest class first"


@pytest.mark.parametrize("second", [False, True])
def test_sort_border_lengths_random_numbers(second):
    assert sorted({merge_passes(x) for x in BORDER_LENGTHS}) == [0, 1, 2, 3, 4, 5, 6]     # every pass count, both buffer parities
    assert merge_passes(MAX_KEPT) == 6 and merge_passes(3 * CHUNK) == 2 and merge_passes(CHUNK + 1) == 1 and merge_passes(CHUNK) == 0
    rng = np.random.default_rng(100 + second)
    lists = [random_numbers(rng, x) for x in BORDER_LENGTHS]
    check_order_sort(lists, len(lists), second, rng)


def pattern(rng, kind, length):
    if kind == "ascending":
        return np.sort(random_numbers(rng, length))
    if kind == "descending":
        return np.sort(random_numbers(rng, length))[::-1].copy()
    if kind == "equal":
        return np.full(length, int(rng.integers(0, 0xFFFFFFFF)), np.uint32)
    if kind == "two":
        return rng.choice(np.array([7, 0xFFFFFFFE], np.uint32), length)
    if kind == "blocks":                                           # blocks of duplicates, their values in random order
        reps = rng.integers(1, 70, length)
        return np.repeat(random_numbers(rng, length), reps)[:length]
    if kind == "ends":                                             # clustered at 0 and at the largest legal key
        return np.where(rng.integers(0, 2, length) == 1, 0xFFFFFFFE - rng.integers(0, 3, length), rng.integers(0, 3, length)).astype(np.uint32)
    # one side of the last merge empty for whole tiles: everything before the last power-of-two border below / above everything behind it
    cut = 1 << (max(length - 1, 1).bit_length() - 1)
    lowpart, high = rng.integers(0, 1 << 31, length, dtype=np.uint64), rng.integers(1 << 31, 0xFFFFFFFF, length, dtype=np.uint64)
    first_low = kind == "a_below_b"
    return np.concatenate(((lowpart if first_low else high)[:cut], (high if first_low else lowpart)[cut:])).astype(np.uint32)


PATTERNS = ["ascending", "descending", "equal", "two", "blocks", "ends", "a_below_b", "b_below_a"]
PATTERN_LENGTHS = [1, 16, 17, 2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385, 32768, 32769, 49152, 49153, 65537, 131073, 262145]


@pytest.mark.parametrize("second", [False, True])
def test_sort_contents_on_both_sides_of_each_border(second):
    rng = np.random.default_rng(200 + second)
    lists = [pattern(rng, kind, x) for kind in PATTERNS for x in PATTERN_LENGTHS]
    lists += [pattern(rng, kind, MAX_KEPT) for kind in ("descending", "a_below_b", "b_below_a")]
    assert all(len(x) == want for x, want in zip(lists, PATTERN_LENGTHS * len(PATTERNS)))
    check_order_sort(lists, len(lists) + 5, second, rng)


@pytest.mark.parametrize("second", [False, True])
def test_sort_more_short_lists_than_blocks(second):
    rng = np.random.default_rng(300 + second)
    lens = np.concatenate((rng.integers(1, 2049, 6000), [1, 2048, 2048, 1, 16, 17]))
    assert len(lens) >= 5000 and len(lens) > 256 * 16 and lens.max() == 2048       # more lists than the 128-thread instance's 4 096 blocks
    check_order_sort([random_numbers(rng, int(x)) for x in lens], len(lens), second, rng)


@pytest.mark.parametrize("second", [False, True])
def test_sort_more_chunks_and_tiles_than_blocks(second):
    rng = np.random.default_rng(400 + second)
    lens = np.concatenate((rng.integers(8193, 16385, 300), rng.integers(16385, 49153, 150), rng.integers(300000, 500000, 12), [8193, 16384, 16385]))
    items = sum(-(-int(x) // CHUNK) for x in lens if x > WHOLE_MAX)
    tiles = sum(-(-int(x) // TILE) for x in lens if x > CHUNK)
    assert items > 512 and tiles > 2048, (items, tiles)            # the chunk grid is 512 blocks, the merge grid 2 048
    check_order_sort([random_numbers(rng, int(x)) for x in lens], len(lens), second, rng)


def mixed_lengths(rng, count, without=None):
    classes = {"short": (1, 2049), "mid": (2049, 4097), "long": (4097, 8193), "chunk": (8193, 16385), "merged": (16385, 70000)}
    names = [k for k in classes if k != without]
    lens = [int(rng.integers(*classes[names[i % len(names)]])) for i in range(count)]
    return lens


@pytest.mark.parametrize("second", [False, True])
def test_sort_mixed_classes_in_shuffled_order_and_sparse_batches(second):
    rng = np.random.default_rng(500 + second)
    lens = mixed_lengths(rng, 400) + [2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385]
    lists = [random_numbers(rng, x) for x in lens]
    check_order_sort(lists, len(lists), second, rng)               # the batch is the lists
    check_order_sort(lists[:60], 100000, second, rng)              # a batch much larger than its sorted class
    check_order_sort(lists[:3], 4097, second, rng)


@pytest.mark.parametrize("second", [False, True])
def test_sort_single_list_calls(second):
    rng = np.random.default_rng(600 + second)
    for x in (1, 2, 2048, 2049, 8192, 8193, 16384, 16385, 100000):
        check_order_sort([random_numbers(rng, x)], 1, second, rng)
    check_order_sort([random_numbers(rng, 40000)], 1000, second, rng)


@pytest.mark.parametrize("without", ["short", "mid", "long", "chunk", "merged"])
def test_sort_with_one_class_empty(without):
    rng = np.random.default_rng(len(without) * 31)
    lens = mixed_lengths(rng, 80, without)
    border = {"short": (1, 2048), "mid": (2049, 4096), "long": (4097, 8192), "chunk": (8193, 16384), "merged": (16385, MAX_KEPT)}[without]
    assert not any(border[0] <= x <= border[1] for x in lens)
    check_order_sort([random_numbers(rng, x) for x in lens], len(lens) + 3, without in ("mid", "chunk"), rng)
    only = {"short": (1, 2049), "mid": (2049, 4097), "long": (4097, 8193), "chunk": (8193, 16385), "merged": (16385, 40000)}[without]
    check_order_sort([random_numbers(rng, int(rng.integers(*only))) for _ in range(20)], 20, False, rng)   # ... and that class alone


# ======================================================================================================================
# gw_sorted_cands_kernel against the oracle's candidates on the same (target << 32 | window) list
# ======================================================================================================================
NT = 600
GAP = C["kGwGap"]


def _table():
    rng = np.random.default_rng(11)
    w = rng.integers(40, 3000, NT)
    w[0::7] = 1                       # targets with one window (the first target of the table is one)
    w[1::7] = 6000                    # targets that hold long dense runs
    tax = 1 + np.arange(NT) // 3      # three neighbouring targets per taxon ...
    tax[np.arange(NT) % 11 == 7] = 0  # ... and some targets without one
    return kh.GwLayout(w, GAP), tax.astype(np.uint32)


LAY, TAX = _table()
WIDE = [t for t in range(NT) if t % 7 == 1]
ONEWIN = [t for t in range(NT) if t % 7 == 0]


class Case:
    def __init__(self, name, segs, max_win, kind="strong"):
        segs = sorted(((int(t), np.asarray(w, dtype=np.int64)) for t, w in segs), key=lambda s: s[0])
        ts = [t for t, _ in segs]
        assert len(set(ts)) == len(ts), name
        for t, w in segs:
            assert len(w) and np.all(np.diff(w) >= 0) and w[0] >= 0 and w[-1] < LAY.windows[t], (name, t)
        self.name, self.max_win, self.kind = name, int(max_win), kind
        self.gw = np.concatenate([LAY.numbers(np.full(len(w), t), w) for t, w in segs])
        self.ends = np.cumsum([len(w) for _, w in segs]) - 1       # list positions where the target runs end
        assert np.all(np.diff(self.gw.astype(np.int64)) >= 0) and 1 <= self.max_win <= GAP


def run(rng, t, length, span=None, w0=None):
    """`length` locations of target t: random windows of a span (1: the same window again and again), ascending"""
    W = int(LAY.windows[t])
    span = W if span is None else max(1, min(int(span), W))
    w0 = int(rng.integers(0, W - span + 1)) if w0 is None else w0
    assert w0 + span <= W
    return t, np.sort(rng.integers(w0, w0 + span, length))


def supports(rng, lo, hi, max_win, count=5):
    """`count` targets strictly between lo and hi, in distinct taxa, with 2 .. 6 locations inside one window range each"""
    groups = sorted({t // 3 for t in range(lo + 1, hi)})
    segs = []
    for g in rng.permutation(groups):
        ts = [t for t in range(3 * g, 3 * g + 3) if lo < t < hi and TAX[t] != 0]
        if ts and len(segs) < count:
            segs.append(run(rng, int(rng.choice(ts)), int(rng.integers(2, 7)), span=1 if rng.integers(0, 2) else max_win))
    assert len(segs) == count
    return segs


def by_lengths(rng, name, seglens, max_win, lo_t=1, hi_t=520, span=None, tail=True, kind="strong"):
    """target runs of the given lengths from list position 0 on (so the places of their ends are known), the supporting targets behind them"""
    seglens = [int(x) for x in seglens if x > 0]
    ts = np.sort(rng.choice(np.arange(lo_t, hi_t), len(seglens), replace=False))
    segs = [run(rng, int(t), L, span=(span if span is not None else int(rng.choice([1, 4, max_win, 3 * max_win, 6000])))) for t, L in zip(ts, seglens)]
    if tail:
        segs += supports(rng, int(ts[-1]), NT, max_win)
    return Case(name, segs, max_win, kind)


def block_borders(n):
    """list positions where the sixteen waves' runs of the block instance begin"""
    chunks = -(-n // 64)
    cpw = -(-chunks // 16)
    return [w * cpw * 64 for w in range(1, 16) if w * cpw * 64 < n], cpw


def straddling(rng, name, n, max_win):
    """a block-instance list of exactly n numbers whose target runs end just before, at and just behind the waves' borders, some runs
    covering several waves, with window ranges that begin before a wave's run"""
    tail = supports(rng, 540, NT, max_win)
    nfeat = n - sum(len(w) for _, w in tail)
    borders, cpw = block_borders(n)
    cuts = set(int(x) for x in rng.integers(1, nfeat, 25))
    for i, b in enumerate(borders):
        if i % 5 != 3:                                             # (every fifth border lies inside a run that covers two waves' pieces)
            cuts.add(b + [-2, -1, 0, 1, 2, 63, 64, -64, -63][i % 9])
    cuts = sorted(c for c in cuts if 0 < c < nfeat)
    seglens = np.diff([0] + cuts + [nfeat])
    ts = np.sort(rng.choice(np.arange(1, 540), len(seglens), replace=False))
    segs = [run(rng, int(t), int(L), span=int(rng.choice([1, max_win, 6000]))) for t, L in zip(ts, seglens)]
    c = Case(name, segs + tail, max_win)
    assert len(c.gw) == n
    return c


def shape_cases(rng):
    cases = []
    # target runs that end at the last lanes of a chunk, at a chunk's first lanes, at the ring's wrap
    for p in (62, 63, 64, 65, 127, 128, 129):
        cases.append(by_lengths(rng, f"run ends at {p}, same window", [p + 1, 3, 70], 2, span=1))
        cases.append(by_lengths(rng, f"run ends at {p}, dense", [p + 1, 3, 70], 40, span=200))
        assert cases[-1].ends[0] == p
    # one target over three and more whole chunks (the chunk lies inside the open target)
    for L, mw in ((300, 16), (1000, 1024), (5000, 100)):
        segs = [run(rng, 3, 10, span=5), run(rng, WIDE[2], L, span=3000), run(rng, WIDE[2] + 1, 7, span=3)]
        cases.append(Case(f"one target over {L} places", segs + supports(rng, WIDE[2] + 1, NT, mw), mw))
    # window ranges of 1, 63, 64, 65, 128, 129 and about 1 000 list elements: the same window repeated ...
    for m in (1, 63, 64, 65, 128, 129, 1000):
        w = 3000
        wins = np.concatenate(([w - 2], np.full(m, w), [w + 2]))
        cases.append(Case(f"window repeated {m} times", [(WIDE[5], wins), run(rng, 2, 3, span=1)] + supports(rng, WIDE[5], NT, 2), 2))
    # ... and dense windows, maxWin from 1 to the gap: every range holds maxWin elements
    for mw in (1, 2, 63, 64, 65, 128, 129, 1000, GAP):
        wins = 100 + np.arange(2000)
        cases.append(Case(f"dense windows, maxWin {mw}", [(WIDE[7], wins), run(rng, 5, 4, span=2)] + supports(rng, WIDE[7], NT, mw), mw))
    # maxWin - 1 equal to a difference in the list (inside the range), and maxWin equal to it (outside)
    for d in (1, 5, 63, 1023):
        for mw in (d + 1, d):
            wins = 50 + d * np.arange(4)
            cases.append(Case(f"difference {d}, maxWin {mw}", [(WIDE[9], wins), (WIDE[10], np.repeat(wins, 2))] + supports(rng, WIDE[10], NT, mw), mw))
    # equal hits across targets (neighbours share a taxon): the lower target wins
    segs = [run(rng, t, 3, span=1) for t in range(200, 209)]
    cases.append(Case("equal hits across nine targets", segs + supports(rng, 209, NT, 4), 4))
    segs = [run(rng, t, 70, span=1) for t in range(210, 216)]
    cases.append(Case("equal hits across six targets of 70", segs + supports(rng, 216, NT, 4), 4))
    # equal hits at two places of one target: the first wins -- neighbours, a chunk apart, many chunks apart
    for between in (0, 3, 80, 400):
        wins = np.concatenate(([10, 11, 12, 13], 100 + 9 * np.arange(between), [5000, 5001, 5002, 5003]))
        cases.append(Case(f"equal hits twice, {between} between", [(WIDE[11], wins)] + supports(rng, WIDE[11], NT, 8), 8))
    # a later window range with more hits, chunks behind the target's first best
    wins = np.concatenate(([10, 11, 12], 100 + 9 * np.arange(100), [3000, 3001, 3002, 3003, 3004]))
    cases.append(Case("later range with more hits", [(WIDE[13], wins), run(rng, WIDE[13] + 1, 2, span=1)] + supports(rng, WIDE[13] + 1, NT, 8), 8))
    # the first and the last target of the table, targets with one window
    segs = [(0, [0, 0, 0]), (ONEWIN[1], np.zeros(70, np.int64)), (ONEWIN[3], [0, 0]), (NT - 1, np.sort(rng.integers(0, LAY.windows[NT - 1], 4)))]
    cases.append(Case("first and last target, one-window targets", segs + supports(rng, ONEWIN[3], NT - 1, 1024), 1024))
    cases.append(Case("only the last target and supports", [run(rng, NT - 1, 9, span=3)] + supports(rng, 0, NT - 1, 3), 3))
    # 8 192 numbers (the longest list of the one-wave instance) and 8 193 (the shortest of the block instance)
    for n in (BIG_SORTED - 1, BIG_SORTED, BIG_SORTED + 1):
        tail = supports(rng, 520, NT, 16)
        left = n - sum(len(w) for _, w in tail)
        lens = []
        while sum(lens) < left:
            lens.append(min(int(rng.choice([1, 2, 5, 64, 65, 300, 1500])), left - sum(lens)))
        c = by_lengths(rng, f"{n} numbers", lens, 16, tail=False)
        cases.append(Case(f"{n} numbers", [(t, w) for t, w in _segments(c)] + tail, 16))
        assert len(cases[-1].gw) == n
    # block-instance lists: runs and ranges across the waves' borders; 8 193 numbers leave the sixteenth wave without a chunk
    for n, mw in ((8193, 1024), (8200, 2), (9000, 64), (12345, 1024), (16389, 300), (40000, 1024), (100001, 17)):
        cases.append(straddling(rng, f"block list of {n}", n, mw))
    borders, cpw = block_borders(8193)
    assert len(borders) == 14 and 15 * cpw * 64 >= 8193            # (fewer than sixteen CHUNKS never reach the block instance: 8 193 numbers are 129)
    return cases


def _segments(case):
    t, w = LAY.split(case.gw)
    cut = np.flatnonzero(np.diff(t.astype(np.int64))) + 1
    return [(int(tt[0]), ww) for tt, ww in zip(np.split(t, cut), np.split(w.astype(np.int64), cut))]


def weak_cases(rng, K, tax):
    cases = []
    ts = np.sort(rng.choice(np.arange(NT), 30, replace=False))
    cases.append(Case("one location per target", [run(rng, int(t), 1) for t in ts], 16, "weak"))
    # a block-instance list without any range of two: windows two apart, maxWin 2
    segs = [(t, 10 + 50 * np.arange(110)) for t in WIDE]
    cases.append(Case("block list of single hits", segs, 2, "weak"))
    assert len(cases[-1].gw) > BIG_SORTED
    cases.append(Case("one-wave list of single hits", segs[:40], 50, "weak"))
    if K >= 2:                                                     # K - 1 targets with a range of two or more, single hits elsewhere
        strong = [run(rng, t, 4, span=1) for t in (100, 130, 160)[:K - 1]]
        cases.append(Case(f"{K - 1} strong targets", strong + [run(rng, t, 1) for t in (300, 303, 306, 309, 312)], 8, "weak"))
        cases.append(Case(f"{K - 1} strong targets, long", strong + [(t, 10 + 50 * np.arange(110)) for t in WIDE if t > 200], 8, "weak"))
        cases.append(Case(f"{K - 1} targets in all", strong, 8, "weak"))
    if tax and K >= 2:                                             # K + 1 and more strong targets in fewer than K taxa
        segs = [run(rng, t, 5, span=1) for g in range(K - 1) for t in (30 + 3 * g, 31 + 3 * g, 32 + 3 * g) if TAX[t]]
        cases.append(Case("strong targets in too few taxa", segs, 8, "weak"))
    if tax:                                                        # strong targets without a taxon are no candidates at all
        none = [t for t in range(NT) if TAX[t] == 0]
        cases.append(Case("strong targets without taxon", [run(rng, t, 6, span=1) for t in none[:8]], 8, "weak"))
        cases.append(Case("strong targets without taxon, long", [run(rng, t, 400, span=1) for t in none[:25]], 8, "weak"))
    return cases


def check_sorted_cands(cases, K, tax, n, rng):
    """one call for all cases; -> midCount[kCntSortedBig]"""
    orc = cpuref.oracle()
    tk64 = TAX.astype(np.int64) if tax else None
    expected = []
    for c in cases:                                                # on the CPU first: the oracle's answer is what the case was built for
        o = orc.candidates(LAY.locations(c.gw), c.max_win, K, tk64, merge=tax)
        strong = len(o) == K and bool(np.all(o["hits"] >= 2))
        assert strong == (c.kind == "strong"), (c.name, c.kind, K, tax, o)
        expected.append(o)
    lengths, offsets, pool = kh.pack_lists([c.gw for c in cases])
    q = rng.permutation(n)[:len(cases)]
    qhits = lengths + rng.integers(0, 5000, len(cases)).astype(np.uint32)
    cands, qflag, hitscan, big = kh.sorted_cands(n, lengths, offsets, pool, [c.max_win for c in cases], q, qhits, LAY, K, TAX if tax else None)
    bad = []
    for i, (c, o) in enumerate(zip(cases, expected)):
        qi = int(q[i])
        if c.kind == "strong":
            if qflag[qi] != C["kFlagDone"]:
                bad.append((c.name, "qflag", int(qflag[qi])))
            for f in kh.cand_fields:
                if not np.array_equal(cands[qi][f], o[f]):
                    bad.append((c.name, f, cands[qi][f].tolist(), o[f].tolist()))
        else:
            if qflag[qi] != C["kFlagCands"] or hitscan[qi] != qhits[i]:
                bad.append((c.name, "weak", int(qflag[qi]), int(hitscan[qi]), int(qhits[i])))
    rest = np.setdiff1d(np.arange(n), q)
    if len(rest) and not (np.all(qflag[rest] == kh.UNTOUCHED32) and np.all(hitscan[rest] == kh.UNTOUCHED32) and np.all(cands[rest]["hits"] == 0xFFFFFFFF)):
        bad.append(("reads without a list were written",))
    assert not bad, (K, tax, n, bad[:8])
    return big


@pytest.mark.parametrize("tax", [False, True])
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_sorted_scan_shapes_against_the_oracle(K, tax):
    rng = np.random.default_rng(1000 + 10 * K + tax)
    cases = shape_cases(rng) + weak_cases(rng, K, tax)
    order = rng.permutation(len(cases))
    cases = [cases[i] for i in order]
    nbig = sum(len(c.gw) > BIG_SORTED for c in cases)
    assert 5 <= nbig < FEW_BIG
    big = check_sorted_cands(cases, K, tax, len(cases) + 37, rng)
    assert big == nbig                                             # the block instance took exactly the lists beyond 8 192 numbers


@pytest.mark.parametrize("K,tax", [(2, False), (3, True)])
def test_sorted_scan_more_big_lists_than_the_block_instance_takes(K, tax):
    rng = np.random.default_rng(2000 + K)
    cases = []
    for i in range(1030):
        n = int(rng.integers(8200, 8301))
        if i % 10 == 9:                                            # every tenth list is weak: single hits only
            wins = 10 + 50 * np.arange(110)
            segs = [(t, wins) for t in WIDE[:n // 110]] + [(WIDE[-1], wins[:n % 110])] * (n % 110 > 0)
            cases.append(Case(f"weak big list {i}", segs, 2, "weak"))
        else:
            cases.append(straddling(rng, f"big list {i}", n, int(rng.choice([2, 16, 300, 1024]))))
        assert len(cases[-1].gw) == n
    big = check_sorted_cands(cases, K, tax, 1030, rng)
    assert big == FEW_BIG == 1024                                  # the cap: the six shortest lists fell back to one wave each


@pytest.mark.parametrize("n", [1, 3, 4, 5, 6000])
def test_sorted_scan_batch_sizes(n):
    rng = np.random.default_rng(3000 + n)                          # (the grid is (n + 3) / 4 blocks of four waves)
    pool = [c for c in shape_cases(rng) if len(c.gw) < 3000]
    k = min(n, 40)
    for K, tax in ((2, False), (4, True)):
        cases = [pool[i] for i in rng.permutation(len(pool))[:k]]
        if n >= 3:
            cases[1] = straddling(rng, "block list", 8193 + n, 64)
            cases[2] = weak_cases(rng, K, tax)[0]
        big = check_sorted_cands(cases, K, tax, n, rng)
        assert big == (1 if n >= 3 else 0)
