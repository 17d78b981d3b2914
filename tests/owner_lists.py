"""Chosen location lists for the owner call of Mode K, mc_candidates_from_partial_numbers (TEST INFRASTRUCTURE, next to
kernel_harness.py and cpuref.py).  The call takes the numbers themselves -- counts[S][n], the sources' blocks, host offsets -- and
runs owner_entries, the whole filtered path of the compact store (gw_filter_count / gw_filter, gw_filter2, gw_compact, the three
gw_filter_stream instances, gw_count<9/10/11>, the sorted tail), decode_union and cands_from_hits on them: a list can be put exactly
on a kernel's border and the result held against the oracle's candidates on the sorted union of the same locations.

    Case              a read: S pieces of global window numbers in any order + maxWindowsInRange, and its shape (H, rounds, kept, distinct)
    route_of(case)    the kernels that filter and finish the read, from the rules in read_class.h and gw_kernels.hip
    handed_back(..)   does the finishing kernel hand the read back to the sort (True / False / None: the model does not say)
    pack(..)          cases at chosen reads of a batch -> counts, numbers, source offsets, max_win; unpack(..) reads them back
    owner_call(..)    the call on a device buffer [trap | payload | 4 words | trap]; check(..) holds everything against the model

Nothing here needs a device until owner_call / context are used (tests/test_owner_lists_cpu.py proves the inputs without one)."""
from __future__ import annotations

import ctypes as C

import numpy as np

import cpuref
from kernel_harness import source_constant

# ---- the kernels' constants: read from the sources where the pattern can, else named literals ---------------------------------
GAP = source_constant("kernels.h", "kGwGap")
MID64 = source_constant("read_class.h", "kMid64")
SMALL_H = source_constant("read_class.h", "kGwSmallH")
HASH_WIN = source_constant("read_class.h", "kHashWin")
REC_ENT_MAX = (1 << source_constant("read_class.h", "kRecEntBits")) - 1          # kRecEntMax
MAX_HITS = (1 << 20) - 1                                                         # read_class.h: kMaxHitsPerQuery
ROUNDS = source_constant("gw_kernels.hip", "kGwRounds")
BIG_H = source_constant("gw_kernels.hip", "kGwBigH")
BIG_SORTED = source_constant("gw_kernels.hip", "kGwBigSorted")
MAX_COUNTED = source_constant("device_common.h", "kBigMaxFilteredCount")
MAX_KEPT = MAX_HITS                                                              # device_common.h: kGwMaxKept = kMaxHitsPerQuery
F2_ROUNDS, F2_H = 2 * ROUNDS, 2 * SMALL_H                                        # gw_filter2_kernel: kMaxRounds, kMaxH
KEEP = {1: 384, 6: 384, 5: 512}                                                  # gw_filter_count_kernel: kKeep of the instances "gw_fuse" 1 / 6 / 5
FUSED_DISTINCT = 256                                                             # ... and kList of its counting (gw_count_read<9, .., LONG>)
COUNT9, COUNT10, COUNT11 = 256, 512, 1024                                        # gw_count_kernel<9 / 10 / 11>: kList
PIECE_MAX = 0xFFFF                                                               # owner_entries_kernel: psize & 0xFFFF
MAX_SOURCES = 64
SLICE_RESERVE = ROUNDS * 16 + 64                                                 # gw_filter_kernel: a slice with less room sends the read on
MC_ERR_INVALID = -1

# ---- the table of targets (the numbering of DeviceTable: gwBase[0] = gap, gwBase[t + 1] = gwBase[t] + windows(t) + gap) ---------
NT = 600


def _table():
    rng = np.random.default_rng(11)
    w = rng.integers(40, 3000, NT)
    w[0::7] = 1                       # targets with one window (the first target of the table is one)
    w[1::7] = 6000                    # targets that hold long dense runs
    tax = 1 + np.arange(NT) // 3      # three neighbouring targets share a taxon ...
    tax[np.arange(NT) % 11 == 7] = 0  # ... and some targets have none
    base = np.zeros(NT + 1, dtype=np.int64)
    base[0] = GAP
    base[1:] = GAP + np.cumsum(w.astype(np.int64) + GAP)
    return w.astype(np.uint32), base, tax.astype(np.uint32)


WINDOWS, BASE, TAX = _table()
assert int(BASE[-1]) < 1 << 32
WIDE = [t for t in range(NT) if t % 7 == 1]
ONEWIN = [t for t in range(NT) if t % 7 == 0]
TRAP_T = WIDE[-1]                     # no case uses this target: the words around the payload lie in it
LAST_CASE_T = TRAP_T - 1
TAX_RANK = 4                          # the one rank the lineages are prepared for
# wide targets of distinct taxa, none without one: K <= 4 strong candidates with and without taxon merging
STRONG_T = [t for t in WIDE if TAX[t] != 0 and t < LAST_CASE_T]
assert len({int(TAX[t]) for t in STRONG_T}) == len(STRONG_T) > 60


def numbers(tgt, win) -> np.ndarray:
    tgt = np.asarray(tgt, dtype=np.int64)
    win = np.asarray(win, dtype=np.int64)
    assert np.all(win >= 0) and np.all(win < WINDOWS[tgt].astype(np.int64))
    return (BASE[tgt] + win).astype(np.uint32)


def split(gw):
    gw = np.asarray(gw, dtype=np.int64)
    tgt = np.searchsorted(BASE, gw, side="right") - 1
    win = gw - BASE[tgt]
    assert np.all(tgt >= 0) and np.all(tgt < NT) and np.all(win < WINDOWS[tgt].astype(np.int64))
    return tgt, win


def locations(gw) -> np.ndarray:
    """numbers -> the oracle's sorted (target << 32 | window) list"""
    t, w = split(np.sort(np.asarray(gw, dtype=np.int64)))
    return (t.astype(np.uint64) << np.uint64(32)) | w.astype(np.uint64)


TRAP = numbers(np.full(3, TRAP_T), [100, 101, 102])          # dense: a word counted outside a piece shows as a candidate
TRAP_SLACK = numbers(np.full(4, TRAP_T), [200, 200, 201, 201])   # the 16 readable bytes behind the payload


# ---- a read ---------------------------------------------------------------------------------------------------------------------
class Case:
    """pieces: S arrays of window numbers, in any order, possibly empty.  The shape:
    H locations; rounds = sum of ceil(c / 16) over the pieces of more than one number; kept_lo = the elements that have another
    element of the read (an equal number counts) less than max_win away -- the block filters never drop those (the neighbour is in the
    same block, or both lie within D of a block edge; the fine-block instance asks the neighbour blocks) -- kept_hi = H; distinct =
    the distinct numbers among the kept_lo elements.  A list in which every element has such a neighbour is kept whole:
    kept_lo == kept_hi, and the Bloom filters' false positives cannot move it."""

    def __init__(self, name, pieces, max_win, named=None):
        self.name, self.max_win = name, int(max_win)
        self.pieces = [np.ascontiguousarray(p, dtype=np.uint32) for p in pieces]
        self.S = len(self.pieces)
        assert 1 <= self.S <= MAX_SOURCES and self.max_win >= 1, name
        self.gw = np.sort(np.concatenate(self.pieces).astype(np.int64))
        split(self.gw)                                              # (every number is some target's window)
        assert not np.any((self.gw >= BASE[TRAP_T]) & (self.gw < BASE[TRAP_T + 1])), name
        self.H = len(self.gw)
        self.rounds = sum(-(-len(p) // 16) for p in self.pieces if len(p) > 1)
        self.pieces_fit = all(len(p) <= PIECE_MAX for p in self.pieces)
        near = np.zeros(self.H, dtype=bool)
        if self.H > 1:
            d = np.diff(self.gw) < self.max_win
            near[1:] |= d
            near[:-1] |= d
        self.kept_lo, self.kept_hi = int(near.sum()), self.H
        self.distinct, self.distinct_hi = len(np.unique(self.gw[near])), len(np.unique(self.gw))
        self.named = dict(named or {})                              # what the case was built for: H, rounds, distinct, route, tuning
        self._exp = {}

    def takes(self) -> bool:
        """owner_entries_kernel: filter_takes with bigMin 0 on a compact store, and no piece beyond 65 535 numbers"""
        return (self.pieces_fit and self.H > MID64 and self.S <= REC_ENT_MAX and self.max_win <= GAP and self.H <= MAX_HITS)

    def expected(self, K, tax):
        """the oracle's candidates on the sorted union (None: more locations than a read may have -- no answer in this library)"""
        if self.H > MAX_HITS:
            return None
        if (K, tax) not in self._exp:
            self._exp[(K, tax)] = cpuref.oracle().candidates(locations(self.gw), self.max_win, K, TAX.astype(np.int64) if tax else None, merge=tax)
        return self._exp[(K, tax)]

    def strong(self, K, tax) -> bool:
        o = self.expected(K, tax)
        return o is not None and len(o) == K and bool(np.all(o["hits"] >= 2))


# ---- the route ------------------------------------------------------------------------------------------------------------------
FINISHERS = ("fused", "count9", "count10", "count11", "sorted_wave", "sorted_block")
# every route the model can name for certain; (route, can the finishing kernel hand the read back)
ROUTES = {"empty": False, "sort": False, "too_many": False, "fused": True,
          "filter>count9": True, "filter>count10": True, "filter>filter2>count10": True, "filter>count11": True, "filter>sorted_wave": True,
          "filter2>sorted_wave": True, "stream>sorted_wave": True, "stream>sorted_block": True, "stream_mid>sorted_wave": True,
          "stream_fine>sorted_wave": True, "stream_fine>sorted_block": True}


def _route(c: Case, n2: int, distinct: int, fuse: int, mid_h: int, big_h: int) -> str:
    if c.H == 0:
        return "empty"
    if c.H > MAX_HITS:
        return "too_many"                                           # read_class.h: no segment, no candidates
    if not c.takes():
        return "sort"                                               # short list, a piece beyond 65 535, a window range beyond the gap
    mw = c.max_win
    big_h = big_h if big_h > 0 else 0xFFFFFFFF                      # mc_set_tuning "gw_big_h" 0: no fine-block instance
    # the head of gw_filter_kernel's / gw_filter_count_kernel's loop (nent <= 64 and maxWin <= gwGap hold for every read taken here)
    if c.H <= SMALL_H and c.rounds <= ROUNDS:
        filt = "filter"
        if fuse and mw <= HASH_WIN and n2 <= KEEP[fuse]:
            if distinct <= FUSED_DISTINCT:
                return "fused"
            # more than 256 distinct: the seven-wave instance has the read filtered again, the others hand the list on through the pool
            return "filter>filter2>count10" if fuse == 1 else "filter>count10"
    elif c.H <= F2_H and c.rounds <= F2_ROUNDS:
        filt = "filter2"
    else:                                                           # gw_filter_stream_kernel's instances by H in (hMin, hMax]
        filt = "stream_fine" if c.H > big_h else "stream_mid" if c.H <= min(mid_h, big_h) else "stream"
    # gw_compact_kernel's class_of / gw_sorted_class, gw_count_kernel's n2 in (minN2, kList]
    if n2 > MAX_COUNTED or mw > HASH_WIN:
        fin = "sorted_block" if n2 > BIG_SORTED else "sorted_wave"
    else:
        fin = "count9" if n2 <= COUNT9 else "count10" if n2 <= COUNT10 else "count11"
    return filt + ">" + fin


def route_of(c: Case, fuse: int = 1, mid_h: int = 0, big_h: int = BIG_H) -> str:
    """which kernels filter and finish the read ("uncertain": the filters' false positives decide -- kept_lo and kept_hi lie on
    different sides of a border).  Pool slices with room are assumed (the pool tests say what they expect themselves)."""
    lo, hi = (_route(c, k, d, fuse, mid_h, big_h) for k, d in ((c.kept_lo, c.distinct), (c.kept_hi, c.distinct_hi)))
    return lo if lo == hi else "uncertain"


def region_picks(c: Case, K: int):
    """gw_pick without taxon merging: K rounds of (most hits, smallest number), the winner's REGION (numbers within the gap) struck
    -> [(number, hits)]"""
    nums, cnt = np.unique(c.gw, return_counts=True)
    cs = np.concatenate(([0], np.cumsum(cnt)))
    R = cs[1:] - cs[np.searchsorted(nums, nums - c.max_win, side="right")]      # hits of the window range that ends in each number
    live = np.ones(len(nums), dtype=bool)
    picks = []
    for _ in range(K):
        if not live.any():
            break
        m = int(R[live].max())
        g = int(nums[live & (R == m)].min())
        picks.append((g, m))
        live &= np.abs(nums - g) > GAP
    return picks


def handed_back(c: Case, route: str, K: int, tax: bool):
    """does the finishing kernel give the read to the sort (its H locations are decoded then)?  None: the model does not say."""
    if route in ("empty", "sort", "too_many"):
        return False
    if route == "uncertain":
        return None
    fin = route.rsplit(">", 1)[-1]
    if fin.startswith("sorted") or tax:
        return not c.strong(K, tax)                                 # fewer than K candidates of two or more hits: the exact kernels
    picks = region_picks(c, K)
    if len(picks) == K and all(h >= 2 for _, h in picks):
        t, _ = split([g for g, _ in picks])
        return len(set(t.tolist())) < K                             # two winners of one target (two regions more than the gap apart)
    return None                                                     # step D finishes the read unless a lane cannot vouch for its minimum


# ---- the pool of the filtered lists (query_rules.h: owner_numbers_pool; kernels.hip: big_filter_grid) ---------------------------
POOL_MAX = 0xFFFFFFF0                                                            # query_rules.h: kPoolMax
FILTER_BPC = 48                                                                  # kernels.hip: big_filter_grid, compact store


def filter_grid(n, filter_bpc=0):
    """blocks of four waves of the filter kernels; the pool is cut into one slice per wave"""
    return min(256 * (filter_bpc if filter_bpc > 0 else FILTER_BPC), (n + 3) // 4)


def pool_sizes(n, total, filter_bpc=0):
    """-> (slices, numbers per slice, numbers of the overflow region) of a call with n reads and `total` numbers"""
    grid = filter_grid(n, filter_bpc)
    per_wave = min(131072, max(4096, total // max(n, 1)))                        # wave_slice
    pool = min(POOL_MAX, max(max(n * 448, total // 2), grid * 4 * per_wave))     # filter_pool
    ovf = min(POOL_MAX - pool, max(pool // 4, 8 << 20))
    return 4 * grid, pool // (4 * grid), ovf


# ---- builders -------------------------------------------------------------------------------------------------------------------
def dense(rng, total, distinct, max_win, targets=None, ntargets=6):
    """`total` numbers, `distinct` distinct ones, in runs of consecutive windows of `ntargets` wide targets of distinct taxa: every
    element has a neighbour less than max_win away (max_win 1: an equal number)"""
    if targets is None:
        targets = sorted(int(t) for t in rng.choice(STRONG_T, ntargets, replace=False))
    nt = len(targets)
    per = np.full(nt, distinct // nt)
    per[:distinct % nt] += 1
    assert per.min() >= 1 and per.max() <= 5000 and total >= distinct
    vals = np.concatenate([numbers(np.full(d, t), int(rng.integers(0, 6000 - d)) + np.arange(d)) for t, d in zip(targets, per)]).astype(np.int64)
    need = np.ones(distinct, dtype=np.int64)
    alone = np.repeat(per == 1, per) | (max_win == 1)
    need[alone] = 2
    assert need.sum() <= total, (total, distinct, max_win)
    extra = rng.multinomial(total - int(need.sum()), np.full(distinct, 1.0 / distinct))
    out = np.repeat(vals, need + extra)
    assert len(out) == total
    return out.astype(np.uint32)


def cut(rng, gw, sizes):
    """the numbers in random order, cut into pieces of the given sizes"""
    sizes = [int(s) for s in sizes]
    assert sum(sizes) == len(gw), (sum(sizes), len(gw))
    g = np.asarray(gw, dtype=np.uint32)[rng.permutation(len(gw))]
    return np.split(g, np.cumsum(sizes)[:-1]) if len(sizes) > 1 else [g]


def even(total, S):
    s = np.full(S, total // S)
    s[:total % S] += 1
    return s.tolist()


def case(rng, name, sizes, max_win, distinct=None, route=None, targets=None, ntargets=6, **tuning):
    """a list that is kept whole, in pieces of the given sizes"""
    H = int(sum(sizes))
    d = distinct if distinct is not None else max(2 * ntargets, min(H // 3, 240)) if max_win > 1 else max(ntargets, min(H // 3, 240))
    gw = dense(rng, H, d, max_win, targets, ntargets) if H else np.zeros(0, np.uint32)
    named = dict(H=H, rounds=sum(-(-s // 16) for s in sizes if s > 1), route=route, tuning=tuning)
    if distinct is not None:
        named["distinct"] = distinct
    return Case(name, cut(rng, gw, sizes), max_win, named)


def segments(rng, name, segs, max_win, S, fill=0, route=None):
    """(target, windows) runs as in test_gpu_sorted_kernels.shape_cases, and `fill` further targets of two equal locations each (fewer
    hits than the runs under test, enough locations for the filtered path), in S pieces"""
    used = {int(t) for t, _ in segs}
    gw = [numbers(np.full(len(w), t), w) for t, w in segs]
    free = [t for t in range(2, LAST_CASE_T) if t not in used and t % 7 > 1 and TAX[t] != 0]
    for t in rng.choice(free, fill, replace=False):
        gw.append(numbers([t, t], np.full(2, int(rng.integers(0, WINDOWS[t])))))
    gw = np.concatenate(gw)
    return Case(name, cut(rng, gw, even(len(gw), S)), max_win, dict(H=len(gw), route=route, tuning={}))


def singles(rng, count, exclude=()):
    """one location in each of `count` targets, far from everything else of the read"""
    free = [t for t in range(2, LAST_CASE_T) if t not in exclude and t % 7 > 1]
    ts = rng.choice(free, count, replace=False)
    return numbers(ts, [int(rng.integers(0, WINDOWS[t])) for t in ts])


def border_cases(rng):
    """every border of the owner entries and the filter / counting kernels from both sides; every list is kept whole"""
    c = []
    # ---- owner entries
    c.append(case(rng, "H 64", even(64, 4), 4, route="sort"))
    c.append(case(rng, "H 65", even(65, 4), 4, route="fused"))
    c.append(case(rng, "pieces of 0 1 2 15 16 17 30", [0, 1, 2, 15, 16, 17, 30], 6, route="fused"))
    c.append(case(rng, "pieces of 1 only and one list", [1] * 40 + [41], 3, route="fused"))
    c.append(case(rng, "piece of 65 535", [65535], 16, distinct=3000, route="stream_fine>sorted_block"))
    c.append(case(rng, "piece of 65 536", [65536], 16, distinct=3000, route="sort"))
    c.append(case(rng, "piece of 65 536 beside short ones", [70, 65536, 3], 4, distinct=3000, route="sort"))
    c.append(case(rng, "pieces of 4 000", [4000, 4000, 4000], 40, distinct=2000, route="stream>sorted_block"))
    # (the longest read that has an answer: 16 x 65 535 = kMaxHitsPerQuery - 15 locations; it also gives the call's pool slices their room)
    c.append(case(rng, "16 pieces of 65 535", [65535] * 16, 16, distinct=6000, route="stream_fine>sorted_block"))
    for S in (1, 2, 3, 63, 64):
        c.append(case(rng, f"{S} pieces", even(200, S), 5, route="fused"))
    # ---- register filters: locations, rounds, pieces (four targets of two windows each: with K = 4 every location is in the answer's hits,
    # so a round that is not read shows whichever numbers it held)
    c.append(case(rng, "H 2 048 in 128 rounds", [32] * 64, 7, distinct=8, ntargets=4, route="filter>sorted_wave"))
    c.append(case(rng, "H 2 049 in 128 rounds", [32] * 61 + [48, 48, 1], 7, distinct=8, ntargets=4, route="filter2>sorted_wave"))
    c.append(case(rng, "128 rounds", [17] * 64, 7, distinct=8, ntargets=4, route="filter>sorted_wave"))
    c.append(case(rng, "129 rounds", [17] * 63 + [33], 7, distinct=8, ntargets=4, route="filter2>sorted_wave"))
    # ---- window ranges
    c.append(case(rng, "maxWin 8", even(300, 7), 8, route="fused"))
    c.append(case(rng, "maxWin 9", even(300, 7), 9, route="filter>sorted_wave"))
    c.append(case(rng, "maxWin 1 024", even(300, 7), GAP, route="filter>sorted_wave"))
    c.append(case(rng, "maxWin 1 025", even(300, 7), GAP + 1, route="sort"))
    c.append(case(rng, "maxWin 1", even(300, 7), 1, route="fused"))
    c.append(case(rng, "maxWin 2", even(300, 7), 2, route="fused"))
    # ---- kept numbers (the routes of "gw_fuse" 1; the GPU test runs 6, 5 and 0 as well and asks route_of for each)
    for kept, route in ((256, "fused"), (257, "fused"), (384, "fused"), (385, "filter>count10"), (512, "filter>count10"), (513, "filter>count11"),
                        (1024, "filter>count11"), (1025, "filter>sorted_wave")):
        c.append(case(rng, f"kept {kept}", even(kept, 11), 8, route=route))
    c.append(case(rng, "kept 384, 256 distinct", even(384, 9), 4, distinct=256, route="fused"))
    c.append(case(rng, "kept 384, 257 distinct", even(384, 9), 4, distinct=257, route="filter>filter2>count10"))
    c.append(case(rng, "kept 257, all distinct", even(257, 9), 4, distinct=257, route="filter>filter2>count10"))
    # ---- gw_filter2
    c.append(case(rng, "256 rounds", [50] * 64, 12, distinct=8, ntargets=4, route="filter2>sorted_wave"))
    c.append(case(rng, "257 rounds", [50] * 63 + [65], 12, distinct=8, ntargets=4, route="stream>sorted_wave"))
    c.append(case(rng, "H 4 096 in 256 rounds", [64] * 64, 3, distinct=8, ntargets=4, route="filter2>sorted_wave"))
    c.append(case(rng, "H 4 097 in 256 rounds", [64] * 62 + [128, 1], 3, distinct=8, ntargets=4, route="stream>sorted_wave"))
    # ---- stream filter
    c.append(case(rng, "just past gw_filter2, 64 pieces", [70] * 64, 100, distinct=1500, route="stream>sorted_wave"))
    c.append(case(rng, "H 32 768", [32768], 20, distinct=3000, route="stream>sorted_block"))
    c.append(case(rng, "H 32 769", [32769], 20, distinct=3000, route="stream_fine>sorted_block"))
    c.append(case(rng, "H 8 192, gw_mid_h 8 192", even(8192, 5), 30, distinct=2500, route="stream_mid>sorted_wave", mid_h=8192))
    c.append(case(rng, "H 8 193, gw_mid_h 8 192", even(8193, 5), 30, distinct=2500, route="stream>sorted_block", mid_h=8192))
    c.append(case(rng, "H 5 000, gw_big_h 2 048", even(5000, 3), 30, distinct=2500, route="stream_fine>sorted_wave", big_h=2048))
    return c


def tie_cases(rng):
    """the tie rules of test_gpu_sorted_kernels.shape_cases that fit in a short list, through the fused counting (maxWin <= 8)"""
    c = []
    same = lambda t, k: (t, np.full(k, int(rng.integers(0, WINDOWS[t]))))
    c.append(segments(rng, "equal hits across nine targets", [same(t, 3) for t in range(200, 209)], 4, 7, fill=20, route="fused"))
    for between in (0, 3, 30):
        wins = np.concatenate(([10, 11, 12, 13], 100 + 9 * np.arange(between), [5000, 5001, 5002, 5003]))
        c.append(segments(rng, f"equal hits twice in one target, {between} between", [(WIDE[11], wins)], 8, 5, fill=32, route="fused"))
    wins = np.concatenate(([10, 11, 12], 100 + 9 * np.arange(20), [3000, 3001, 3002, 3003, 3004]))
    c.append(segments(rng, "later range with more hits", [(WIDE[13], wins), same(WIDE[13] + 1, 2)], 8, 6, fill=30, route="fused"))
    segs = [(0, [0, 0, 0]), (ONEWIN[1], np.zeros(5, np.int64)), (ONEWIN[3], [0, 0]), (NT - 1, np.sort(rng.integers(0, WINDOWS[NT - 1], 4)))]
    c.append(segments(rng, "first and last target, one-window targets", segs, 8, 4, fill=30, route="fused"))
    return c


def weak_cases(rng):
    """fewer than K strong targets: everything dense in ONE target (K >= 2 and taxon merging find one candidate of two or more hits),
    single hits in other targets for step D; and lists of single hits only (weak for every K)"""
    c = []

    def one_target(name, sizes, max_win, nsingles, route, distinct=None, **kw):
        H = int(sum(sizes))
        t = int(rng.choice(STRONG_T))
        d = distinct or max(2, min((H - nsingles) // 3, 240))
        gw = np.concatenate((dense(rng, H - nsingles, d, max_win, targets=[t]), singles(rng, nsingles, exclude=(t,))))
        c.append(Case(name, cut(rng, gw, sizes), max_win, dict(H=H, route=route, tuning=kw, weak_from=2)))
    one_target("one strong target, 300 distinct numbers", even(380, 9), 8, 0, "filter>filter2>count10", distinct=300)
    one_target("one strong target and 40 single hits, short", even(64, 3), 8, 40, "sort")
    one_target("one strong target and 40 single hits", even(140, 9), 8, 40, "fused")
    one_target("one strong target, kept 450", even(450, 9), 8, 0, "filter>count10")
    one_target("one strong target, kept 900", even(900, 9), 8, 0, "filter>count11")
    one_target("one strong target, maxWin 50", even(1500, 30), 50, 0, "filter>sorted_wave")
    one_target("one strong target through gw_filter2", [50] * 64, 50, 0, "filter2>sorted_wave")
    one_target("one strong target through the stream filter", even(6000, 2), 50, 0, "stream>sorted_wave")
    one_target("one strong target, block scan", even(9000, 2), 50, 0, "stream>sorted_block")
    one_target("one strong target, fine blocks", [40000], 50, 0, "stream_fine>sorted_block")
    one_target("one strong target, gw_mid_h", even(6000, 2), 50, 0, "stream_mid>sorted_wave", mid_h=8192)
    one_target("one strong target, gw_big_h 2 048", even(6000, 2), 50, 0, "stream_fine>sorted_wave", big_h=2048)
    # single hits only (H <= 384: whatever the filters keep stays inside the fused counting; maxWin 9: the sorted class whatever is kept)
    c.append(Case("single hits only", cut(rng, singles(rng, 150), even(150, 8)), 8, dict(H=150, route="fused", tuning={}, weak_from=1)))
    c.append(Case("single hits only, maxWin 9", cut(rng, singles(rng, 150), even(150, 8)), 9, dict(H=150, route="filter>sorted_wave", tuning={}, weak_from=1)))
    # strong targets without a taxon are no candidates under taxon merging
    none = [t for t in WIDE if TAX[t] == 0 and t < LAST_CASE_T][:5]
    c.append(Case("strong targets without taxon", cut(rng, dense(rng, 200, 60, 6, targets=none), even(200, 6)), 6,
                  dict(H=200, route="fused", tuning={}, weak_from=1, weak_tax_only=True)))
    return c


def two_regions_case(rng):
    """two regions of one target more than the gap apart with the most hits: without taxon merging the counting picks both and hands
    the read back (K >= 2)"""
    t = WIDE[17]
    segs = [(t, np.concatenate((np.full(6, 10), np.full(5, 5000))))]
    return segments(rng, "two regions of one target lead", segs, 8, 5, fill=32, route="fused")


COMBOS = [(1, 0), (2, 0), (4, 0), (1, TAX_RANK), (2, TAX_RANK), (4, TAX_RANK)]       # (K, lowest rank): without and with taxon merging


def too_many_case(rng):
    """more than kMaxHitsPerQuery locations: 17 pieces of 65 535"""
    return case(rng, "17 pieces of 65 535", [65535] * 17, 16, distinct=6000, route="too_many")


def overflow_batch(rng, n=4000, big=100_000):
    """one read of `big` kept numbers among short ones: no slice of the pool can take it -> (cases, their reads, n)"""
    short = [case(rng, f"short {i}", even(80 + 7 * i, 3), 6, route="fused") for i in range(6)]
    long_ = case(rng, f"{big} kept numbers", [50_000, big - 50_000], 30, distinct=6000, route="stream_fine>sorted_block")
    return short[:3] + [long_] + short[3:], [0, 5, n // 2, n // 2 + 1, n // 2 + 2, n - 2, n - 1], n


def full_slices_batch(rng, n=5600, kept=400, filter_bpc=1):
    """thousands of reads that keep `kept` numbers each on a grid cut to filter_bpc blocks per CU: a wave walks several reads, its slice
    fills up, and the later reads are sent on to the stream filter -> (cases, reads, n); the reads share eight lists"""
    kinds = [case(rng, f"{kept} kept, variant {i}", even(kept, 5 + i), 8 if i % 2 == 0 else 30, route=None) for i in range(8)]
    return [kinds[i % 8] for i in range(n)], list(range(n)), n


# ---- packing --------------------------------------------------------------------------------------------------------------------
def pack(cases, at, n, S=None):
    """cases at reads `at` of a batch of n (the other reads have no numbers) -> counts[S * n] source-major, numbers (the sources'
    blocks back to back, each block its reads' pieces in read order), source_offsets[S + 1], max_win[n]"""
    S = max(c.S for c in cases) if S is None else S
    assert len(cases) == len(at) == len(set(int(q) for q in at)) and all(0 <= int(q) < n for q in at) and all(c.S <= S for c in cases)
    counts = np.zeros((S, n), dtype=np.uint32)
    max_win = np.full(n, 3, dtype=np.uint32)
    order = np.argsort(np.asarray(at, dtype=np.int64))
    blocks = []
    for s in range(S):
        for i in order:
            cse, q = cases[i], int(at[i])
            if s < cse.S:
                counts[s, q] = len(cse.pieces[s])
                blocks.append(cse.pieces[s])
    for cse, q in zip(cases, at):
        max_win[int(q)] = cse.max_win
    nums = np.concatenate(blocks + [np.zeros(0, np.uint32)]).astype(np.uint32)
    offsets = np.concatenate(([0], np.cumsum(counts.astype(np.int64).sum(axis=1)))).astype(np.uint64)
    return counts.reshape(-1), nums, offsets, max_win


def unpack(counts, nums, offsets, n):
    """-> per read the list of its S pieces, read back from the arrays the way the header of the call describes them"""
    S = len(offsets) - 1
    counts = np.asarray(counts).reshape(S, n).astype(np.int64)
    out = [[None] * S for _ in range(n)]
    for s in range(S):
        start = int(offsets[s]) + np.concatenate(([0], np.cumsum(counts[s])))
        assert start[-1] == int(offsets[s + 1])
        for q in range(n):
            out[q][s] = nums[start[q]:start[q + 1]]
    return out


# ---- the device side ------------------------------------------------------------------------------------------------------------
def context(K: int):
    """a context with the table of targets, the compact store and lineages for TAX_RANK; the table itself holds a few keys (the owner
    call never looks a feature up) -> api.Database"""
    from metacache_amd import api
    L = api.lib()
    cfg = api.default_config(target_id_bytes=4, max_candidates=K, num_slots=1, slot_max_queries=64, slot_max_chars=1 << 16)
    h = C.c_void_p()
    assert L.mc_create(C.byref(cfg), C.byref(h)) == 0, L.mc_last_error(None)
    db = api.Database.from_handle(h.value, cfg)
    try:
        db.load_target_windows(WINDOWS)
        keys = np.array([11, 12345, 99999, 7], dtype=np.uint32)
        sizes = np.array([1, 2, 3, 1], dtype=np.uint8)
        vals = np.array([[0, 0], [5, 1], [9, 1], [0, 7], [100, 8], [101, 8], [3, NT - 1]], dtype=np.uint32)      # {window, target}
        db._check(L.mc_load_begin(db.h, 0, len(keys), len(vals)))
        db._check(L.mc_load_batch(db.h, 0, keys.ctypes.data, sizes.ctypes.data, vals.ctypes.data, len(keys)))
        db._check(L.mc_load_end(db.h, 0))
        lay = db.table_layout()
        assert lay["location_bytes"] == 4 and lay["window_gap"] == GAP, lay
        lin = np.zeros((NT, 21), dtype=np.uint32)
        lin[:, TAX_RANK] = TAX
        db.set_lineages(lin)
        return db
    except Exception:
        db.close()
        raise


def owner_stats(db) -> np.ndarray:
    """mc_owner_stats: reads, reads on the filtered path, numbers received, locations decoded for the sort"""
    from metacache_amd import api
    L = api.lib()
    L.mc_owner_stats.argtypes = [C.c_void_p, C.c_void_p]
    st = np.zeros(4, dtype=np.uint64)
    db._check(L.mc_owner_stats(db.h, st.ctypes.data))
    return st.astype(np.int64)


def owner_call(db, cases, K, lowest, n=None, order=None, S=None, shift=0):
    """the cases at reads order[i] of a batch of n -> (cands[n, K], qstat[n], delta of mc_owner_stats).  The numbers lie in a larger
    device tensor [trap | payload | 4 words | trap] (the header promises 16 readable bytes behind the end and no more), the payload
    `shift` words behind a 16-byte border"""
    import torch
    from metacache_amd import api
    n = len(cases) if n is None else n
    order = list(range(len(cases))) if order is None else order
    counts, nums, offsets, max_win = pack(cases, order, n, S)
    assert K == db.cfg.max_candidates
    dev = torch.device("cuda", 0)
    lead, tail = 64 + shift, 4096
    buf = np.tile(TRAP, (lead + len(nums) + 4 + tail + 2) // 3 + 1)[:lead + len(nums) + 4 + tail].copy()
    buf[lead:lead + len(nums)] = nums
    buf[lead + len(nums):lead + len(nums) + 4] = TRAP_SLACK
    dbuf = torch.from_numpy(buf.view(np.int32)).to(dev)
    assert dbuf.data_ptr() % 16 == 0
    dcounts = torch.from_numpy(counts.view(np.int32)).to(dev)
    dmw = torch.from_numpy(max_win.view(np.int32)).to(dev)
    before = owner_stats(db)
    res = db.candidates_from_partial_numbers(dcounts.data_ptr(), dbuf.data_ptr() + 4 * lead, offsets, n, max_win_ptr=dmw.data_ptr(), lowest=lowest)
    cands = np.zeros((n, K), dtype=api.cand_dtype)
    qstat = np.zeros(n, dtype=api.qstat_dtype)
    db.copy_results(cands.ctypes.data, res.cands, cands.nbytes, to_host=True)
    db.copy_results(qstat.ctypes.data, res.hit_counts, qstat.nbytes, to_host=True)
    db.synchronize()
    assert np.array_equal(dbuf.cpu().numpy().view(np.uint32), buf), "the call wrote into the numbers"
    return cands, qstat, owner_stats(db) - before


def same_candidates(row, exp) -> bool:
    """a row of K candidates against the oracle's list, padded with empty rows"""
    m = len(exp)
    return (int((row["hits"] > 0).sum()) == m and all(np.array_equal(row[f][:m], exp[f]) for f in ("tgt", "hits", "beg", "end")))


def filter2_room(cases, n, fuse=1, mid_h=0, big_h=BIG_H, filter_bpc=0) -> bool:
    """route_of assumes room in the pool: gw_filter2_kernel takes the records 64 per wave, so at worst ONE slice gets every list it
    keeps, behind one list of gw_filter_kernel's, and needs kMaxRounds x 16 + 64 numbers of room in front of each"""
    f2 = sum(c.kept_hi for c in cases if "filter2" in route_of(c, fuse, mid_h, big_h))
    return f2 == 0 or f2 + SMALL_H + F2_ROUNDS * 16 + 64 <= pool_sizes(n, sum(c.H for c in cases), filter_bpc)[1]


def check(db, cases, K, lowest, n=None, order=None, S=None, shift=0, fuse=1, mid_h=0, big_h=BIG_H, filter_bpc=0, pool_may_hand_back=False):
    """one call; candidates, statistics, owner counters and the sorted tail's timers against the model -> {route: reads}"""
    tax = lowest != 0
    n = len(cases) if n is None else n
    order = list(range(len(cases))) if order is None else [int(q) for q in order]
    S_call = max(c.S for c in cases) if S is None else S
    assert pool_may_hand_back or filter2_room(cases, n, fuse, mid_h, big_h, filter_bpc), "the model's routes assume room in gw_filter2's pool slice"
    for name, v in (("gw_fuse", fuse), ("gw_mid_h", mid_h), ("gw_big_h", big_h), ("filter_bpc", filter_bpc)):
        db.set_tuning(name, v)
    db.timing(True)
    db.timing_reset()
    try:
        cands, qstat, delta = owner_call(db, cases, K, lowest, n, order, S_call, shift)
        ran = {k: db.timing_get(k)[1] for k in ("gw_sort", "gw_sorted_cands", "owner_entries", "decode_union")}
    finally:
        db.timing(False)
        for name, v in (("gw_fuse", 1), ("gw_mid_h", 0), ("gw_big_h", BIG_H), ("filter_bpc", 0)):
            db.set_tuning(name, v)
    bad, reached = [], {}
    taken = decoded_lo = decoded_hi = 0
    sorted_sure = sorted_maybe = False
    for c, q in zip(cases, order):
        route = route_of(c, fuse, mid_h, big_h)
        reached[route] = reached.get(route, 0) + 1
        exp = c.expected(K, tax)
        if exp is None:                                            # more than kMaxHitsPerQuery locations
            if (cands[q]["hits"] != 0).any():
                bad.append((c.name, route, "candidates of a read without an answer", cands[q].tolist()))
        elif not same_candidates(cands[q], exp):
            bad.append((c.name, route, cands[q].tolist(), exp.tolist()))
        if int(qstat[q]["hits"]) != c.H or int(qstat[q]["nfound"]) != S_call:
            bad.append((c.name, route, "qstat", qstat[q].tolist(), c.H, S_call))
        taken += c.takes()
        back = handed_back(c, route, K, tax)
        if route == "sort" or back is True:
            decoded_lo += c.H; decoded_hi += c.H
        elif back is None or (pool_may_hand_back and c.takes()):
            decoded_hi += c.H
        fin = route.rsplit(">", 1)[-1]
        sorted_sure |= fin.startswith("sorted")
        sorted_maybe |= fin.startswith("sorted") or route == "uncertain"
    rest = np.setdiff1d(np.arange(n), np.asarray(order, dtype=np.int64))
    if len(rest) and not ((cands[rest]["hits"] == 0).all() and (qstat[rest]["hits"] == 0).all() and (qstat[rest]["nfound"] == S_call).all()):
        bad.append(("reads without numbers came back with something",))
    total = sum(c.H for c in cases)
    if (int(delta[0]), int(delta[1]), int(delta[2])) != (n, taken, total) or not decoded_lo <= int(delta[3]) <= decoded_hi:
        bad.append(("mc_owner_stats", delta.tolist(), (n, taken, total, decoded_lo, decoded_hi)))
    if (sorted_sure and not (ran["gw_sort"] and ran["gw_sorted_cands"])) or (not sorted_maybe and (ran["gw_sort"] or ran["gw_sorted_cands"])):
        bad.append(("the sorted tail's timers", ran, sorted_sure, sorted_maybe))
    assert not bad, (K, lowest, fuse, mid_h, big_h, n, len(bad), bad[:6])
    return reached
