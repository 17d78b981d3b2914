"""Chosen location lists for the lane hand-over and the read classes of an ordinary query (TEST INFRASTRUCTURE, next to owner_lists.py,
kernel_harness.py and sketch_ref.py).  A read is random ACGT; its features come from the numpy model of the sketch (sketch_ref); the
table holds, for every feature of the read, a list chosen by the case -- so H (locations), the found features (hand-over entries),
singletons against lists, maxWindowsInRange and with them the read's class (read_class.h) are put exactly on a border, and what
db.query returns is held against the oracle's candidates on the sorted union of the same locations.

    Read              sequence(s), feature slots of the numpy sketch, windows, maxWindowsInRange
    Case              a read + a list per feature slot; its model: H, entries, n singletons, m lists, over, handed
    read_class(..)    Python mirror of read_class.h (constants read from the header; pinned against literal rows in the CPU test)
    route_of(case, store, big_min)   the kernel that finishes the read; big_route(case) the 8-byte store's filter -> count / wave
    context(..)       mc_create + mc_load_* of the cases' lists (compact or 8-byte store), lineages of owner_lists' table of targets
    check(..)         ONE db.query (and the same batch through mc_query_device, the call whose statistics mc_last_batch_stats
                      reports): candidates, counts, statistics and the launched timers against the model -> {route: reads}

Nothing here needs a device until context / check are used (tests/test_class_lists_cpu.py proves the inputs without one).

What the model leaves open, and why (each is asserted from the constants in test_class_lists_cpu.py):
  * the ORDER in which a lane meets its found features depends on the hash table's chains (kLaneU lookups in flight); `over`
    (one found feature more than kLaneHits) and, without it, n and m do not -- the candidates never do.
  * kHashEnt 256 / 257 entries: a lane read has at most 2 mates x 5 windows x 16 features = 160 entries.
  * kBigEnt * kBigEPL 192 / 193 entries on the 8-byte store: the same 160.
  * big_setup's rounds of 16 and of 64 lanes with a COUNTED list: r8 <= (H + 7 * entries) / 8 <= 240 for the H <= 1024 the counting
    kernels take from at most 128 entries (maxWin <= kHashWin), so those shapes are only met by reads the filter then hands to the
    wave kernel (kept > kBigMaxFiltered); their candidates are checked all the same.
  * a read beyond kMaxHitsPerQuery: mc_query_device answers it with no candidates; the host's slots refuse the whole batch
    (mc_batch_wait: MC_ERR_UNSUPPORTED), which check() expects of db.query for such a batch.
  * a second trip through mid_cands_kernel's loop over its work list: its grid has a group for every read of the batch
    (ceil(n / (256 / G)) blocks of 256 / G groups); a batch of 256 / G reads of the class fills every group of one block, one read
    more leaves a second block's groups idle but for one.
  * chunk_finish_kernel: 4095 feature slots need an odd sketch length (273 windows x 15), 4096 an even one (256 x 16): the border
    is met from both sides by two contexts, not by two reads of one."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

import cpuref
import owner_lists as ol
import sketch_ref
from kernel_harness import CSRC, source_constant
from owner_lists import NT, STRONG_T, TAX, TAX_RANK, WIDE, WINDOWS, LAST_CASE_T, same_candidates, singles   # noqa: F401 (re-exported)

# ---- the kernels' constants ---------------------------------------------------------------------------------------------------
def _define(file: str, name: str) -> int:
    m = re.search(r"#define\s+" + name + r"\s+(\d+)", open(os.path.join(CSRC, file)).read())
    assert m, (file, name)
    return int(m.group(1))


LANE_HITS = _define("kernels.hip", "MC_LANE_HITS")                               # kLaneHits
CHUNK_WINS = _define("kernels.hip", "MC_CHUNK_WINS")
LANE_MAX_LEN = source_constant("kernels.hip", "kLaneMaxLen")
LANE_S = source_constant("kernels.hip", "kLaneS")
LANE_BLOCK = source_constant("kernels.hip", "kLaneBlock")
LANE_K = source_constant("device_common.h", "kLaneK")
FUSE_CAP = source_constant("kernels.hip", "kFuseCap")
MID_R = source_constant("kernels.hip", "kMidR")
LDS_CAP = source_constant("read_class.h", "kLdsCap")
MID64, MID128, MID_MAX = (source_constant("read_class.h", n) for n in ("kMid64", "kMid128", "kMidMax"))
HASH_MAX, HASH_ENT, HASH_WIN = (source_constant("read_class.h", n) for n in ("kHashMax", "kHashEnt", "kHashWin"))
BIG_ENT, BIG_EPL = source_constant("read_class.h", "kBigEnt"), source_constant("read_class.h", "kBigEPL")
SMALL_H = source_constant("read_class.h", "kGwSmallH")
REC_ENT_MAX = ol.REC_ENT_MAX
MAX_HITS = ol.MAX_HITS
GAP = ol.GAP
BIG_MAX_ROUNDS = BIG_ENT * 4                                                     # kernels.hip: kBigMaxRounds = kBigEnt * 4
BIG_MAX_FILTERED = source_constant("kernels.hip", "kBigMaxFiltered")
BIG_MIN_DEFAULT = 128                                                            # context.h: bigMin
NO_FILTER = 1 << 20                                                              # a big_min no read exceeds (H <= kMaxHitsPerQuery): no filtered path
KMER, WINLEN, STRIDE = 16, 127, 112                                              # mc_config_default; context() asserts them
MAX_LIST = 254                                                                   # longest list a case gives a feature
COMPACT, WIDE8 = "compact", "8-byte"
STORES = (COMPACT, WIDE8)

# class names in the order of read_class.h's numbers 0 .. 7
CLASSES = ("mid64", "mid128", "mid256", "hash512", "hash1024", "hash256", "wave", "filter")
TIMER_OF = {"mid64": "mid_cands_64", "mid128": "mid_cands_128", "mid256": "mid_cands_256", "hash256": "hash_cands_256",
            "hash512": "hash_cands_512", "hash1024": "hash_cands_1024"}


def filter_takes(H, entries, max_win, big_min, compact, gap=GAP):
    if not (H > big_min and H > MID64):
        return False
    if compact:
        return entries <= REC_ENT_MAX and max_win <= gap and H <= MAX_HITS
    return entries <= BIG_ENT * BIG_EPL and max_win <= HASH_WIN


def read_class(H, entries, max_win, big_min, compact, gap=GAP) -> str:
    """read_class.h: read_class()"""
    hash_ok = entries <= HASH_ENT and max_win <= HASH_WIN
    if filter_takes(H, entries, max_win, big_min, compact, gap):
        return "filter"
    if H <= MID64:
        return "mid64"
    if H <= MID128:
        return "hash256" if hash_ok else "mid128"
    if H <= MID_MAX:
        return "hash256" if hash_ok else "mid256"
    if H <= HASH_MAX and hash_ok:
        return "hash512" if H <= HASH_MAX // 2 else "hash1024"
    return "wave"


def filter_second(H, entries, compact) -> bool:
    return H > SMALL_H if compact else entries > BIG_ENT


def segment_hits(H, cls) -> int:
    return H if cls == "wave" and LDS_CAP < H <= MAX_HITS else 0


# ---- a read -------------------------------------------------------------------------------------------------------------------
def random_bases(rng, n) -> bytes:
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)])


class Read:
    """seq1 (+ seq2): the feature slots as the device lays them out (mate 1's windows, then mate 2's, s slots per window, padded
    with 0xFFFFFFFF) from sketch_ref; dup = a window's smallest hashes hold one twice (the lane kernel leaves such a read to the
    wave kernels)"""

    def __init__(self, seq1: bytes, seq2: bytes = b"", s: int = 16):
        self.seq1, self.seq2, self.s = bytes(seq1), bytes(seq2), s
        rows, dup = [], False
        for seq in (self.seq1, self.seq2):
            if len(seq) >= KMER:
                f = sketch_ref.facts(seq, KMER, s, WINLEN, STRIDE)
                rows.append(f.feats)
                dup = dup or bool(f.dup.any())
        self.feats = np.concatenate(rows).reshape(-1) if rows else np.zeros(0, np.uint32)
        self.windows = len(self.feats) // s
        self.dup = dup
        self.max_win = 2 + (len(self.seq1) + len(self.seq2)) // STRIDE               # api.Database.max_windows_in_range
        self.real = np.flatnonzero(self.feats != sketch_ref.NONE)                      # slots that hold a feature
        self.unique = len(set(self.feats[self.real].tolist())) == len(self.real)       # no feature in two windows
        self.chunked = not self.seq2 and len(self.seq1) > LANE_MAX_LEN                 # lane_chunk_records
        self.lane = not dup and len(self.seq1) <= LANE_MAX_LEN and len(self.seq2) <= LANE_MAX_LEN


# ---- a case -------------------------------------------------------------------------------------------------------------------
class Case:
    """a read and, per feature slot, the sorted list of (target << 32 | window) the table holds for that feature (empty: not in the
    table).  named: what the case was built for (the CPU test holds the model against it)."""

    def __init__(self, name, read: Read, lists, named=None):
        self.name, self.read = name, read
        assert len(lists) == len(read.feats), name
        self.lists = [np.asarray(x, dtype=np.uint64) for x in lists]
        self.sizes = np.array([len(x) for x in self.lists], dtype=np.int64)
        assert np.all(self.sizes[read.feats == sketch_ref.NONE] == 0) and self.sizes.max(initial=0) <= MAX_LIST, name
        for x in self.lists:                                       # as the builder writes them: ascending, no location twice
            assert np.all(x[1:] > x[:-1]), name
        self.H = int(self.sizes.sum())
        self.entries = int((self.sizes > 0).sum())
        self.n = int((self.sizes == 1).sum())                      # singletons: the location itself stands in the bucket
        self.m = self.entries - self.n                             # lists: a descriptor at the row's end
        self.over = self.entries > LANE_HITS                       # a found feature arrives at a full row: dump_row, direct entries
        self.handed = self.H > LANE_HITS or self.over
        self.coop = self.handed and not self.over                  # the wave writes the row out
        self.nfeat = len(read.real)
        self.max_win = read.max_win
        self.locs = np.sort(np.concatenate(self.lists + [np.zeros(0, np.uint64)]))
        self.named = dict(named or {})
        self._exp = {}

    def expected(self, K, tax):
        """the oracle's candidates on the sorted union (None: more locations than a read may have)"""
        if self.H > MAX_HITS:
            return None
        if (K, tax) not in self._exp:
            self._exp[(K, tax)] = cpuref.oracle().candidates(self.locs, self.max_win, K, TAX.astype(np.int64) if tax else None, merge=tax)
        return self._exp[(K, tax)]

    def strong(self, K, tax) -> bool:
        o = self.expected(K, tax)
        return o is not None and len(o) == K and bool(np.all(o["hits"] >= 2))

    # -- the hand-over's consumers
    def per(self) -> int:
        return -(-self.H // 64)                                    # hash_cands_kernel: per

    def big_shape(self):
        """big_setup: (r8, r16, shift, R) from the lists of more than one location"""
        big = self.sizes[self.sizes > 1]
        r8, r16 = int((-(-big // 8)).sum()), int((-(-big // 16)).sum())
        shift = 3 if r8 <= BIG_MAX_ROUNDS else 4 if r16 <= BIG_MAX_ROUNDS else 6
        return r8, r16, shift, int((-(-big // (1 << shift))).sum())

    def big_kept(self):
        """(fewest, most) locations big_filter_kernel keeps: its first instance (up to kBigEnt entries) keeps every location whose
        target the read meets twice, the second (POS) every location with another one of its target at most 7 windows away (they
        share a block of 16 in one of the two grids); the Bloom filters may keep any of the rest as well"""
        t, w = (self.locs >> np.uint64(32)).astype(np.int64), (self.locs & np.uint64(0xFFFFFFFF)).astype(np.int64)
        sure = np.zeros(self.H, dtype=bool)
        if self.H > 1:
            if self.entries <= BIG_ENT:
                d = t[1:] == t[:-1]
            else:
                d = (t[1:] == t[:-1]) & (w[1:] - w[:-1] <= 7)
            sure[1:] |= d
            sure[:-1] |= d
        return int(sure.sum()), self.H


def route_of(c: Case, store: str, big_min: int = BIG_MIN_DEFAULT, lane_path: bool = True) -> str:
    """the kernel that finishes the read: "lane", a class of CLASSES, "chunk>filter" / "chunk>wave", "sketch>filter" / "sketch>wave"
    (reads the lane kernel leaves to the wave kernel's sketching: wave_rejoin_kernel's rule), "too_many"."""
    compact = store == COMPACT
    if c.H > MAX_HITS:
        return "too_many"
    if not lane_path:
        return "wave"
    slots = len(c.read.feats)
    if c.read.chunked:                                             # chunk_finish_kernel: the feature slots, found or not, are the entries
        return "chunk>filter" if compact and filter_takes(c.H, slots, c.max_win, big_min, True) else "chunk>wave"
    if not c.read.lane:                                            # wave_rejoin_kernel, compact store only
        return "sketch>filter" if compact and filter_takes(c.H, slots, c.max_win, big_min, True) else "sketch>wave"
    if not c.handed:
        return "lane"
    return read_class(c.H, c.entries, c.max_win, big_min, compact)


def big_route(c: Case) -> str:
    """8-byte store, class filter: "count" (big_count_kernel, up to 512 kept), "count2" (up to 1024), "wave" (more, or more rounds
    than the round table holds), "uncertain" (the Bloom filters' false positives decide)"""
    r8, r16, shift, R = c.big_shape()
    if R > BIG_MAX_ROUNDS:
        return "wave"
    f = lambda k: "count" if k <= HASH_MAX // 2 else "count2" if k <= BIG_MAX_FILTERED else "wave"
    lo, hi = c.big_kept()
    return f(lo) if f(lo) == f(hi) else "uncertain"


# ---- builders -----------------------------------------------------------------------------------------------------------------
SHAPES = {                      # (mate 1, mate 2) -> windows, maxWindowsInRange at the default sketching parameters
    "single150": (150, 0), "single400": (400, 0), "pair250": (250, 250), "pair350": (350, 350), "pair391": (391, 392), "pair400": (400, 400),
    "pair512": (512, 512), "single100": (100, 0),
}


_USED = {}                      # id(rng) -> the features of the reads drawn from it: the reads of one generator share no feature


def claim(rng, r: Read) -> bool:
    """True, and the read's features are taken: none of them is in an earlier read of this generator or twice in this one"""
    used = _USED.setdefault(id(rng), (rng, set()))[1]
    mine = set(r.feats[r.real].tolist())
    if not r.unique or mine & used:
        return False
    used |= mine
    return True


def new_read(rng, shape, s=16) -> Read:
    l1, l2 = SHAPES[shape] if isinstance(shape, str) else shape
    for _ in range(50):
        r = Read(random_bases(rng, l1), random_bases(rng, l2) if l2 else b"", s)
        if not r.dup and claim(rng, r):
            return r
    raise AssertionError("random reads keep repeating a hash")


def _pool(rng, kind, count):
    """`count` distinct locations, sorted: runs of consecutive windows in a few wide targets of distinct taxa ("strong"), in ONE such
    target ("one_target"), in wide targets without a taxon ("no_taxon")"""
    if kind == "one_target":
        targets = [int(rng.choice(STRONG_T))]
    elif kind == "no_taxon":
        targets = [t for t in WIDE if TAX[t] == 0 and t < LAST_CASE_T][:5]
    else:
        targets = sorted(int(t) for t in rng.choice(STRONG_T, 6, replace=False))
    nt = len(targets)
    per = np.full(nt, count // nt)
    per[:count % nt] += 1
    out = []
    for t, d in zip(targets, per):
        first = int(rng.integers(0, 6000 - d))
        out.append((np.uint64(t) << np.uint64(32)) | (first + np.arange(d)).astype(np.uint64))
    return np.sort(np.concatenate(out))


def spread_sizes(rng, H, entries, n_single):
    """sizes of `entries` found features: n_single ones, the others 2 .. MAX_LIST, H in all"""
    m = entries - n_single
    assert 0 <= n_single <= entries and (2 * m <= H - n_single <= MAX_LIST * m), (H, entries, n_single)
    sizes = np.full(m, 2, dtype=np.int64)
    rest = H - n_single - 2 * m
    while rest:                                                    # deal the rest out, a random lot at a time, below the cap
        room = np.flatnonzero(sizes < MAX_LIST)
        j = int(rng.choice(room))
        add = min(rest, MAX_LIST - int(sizes[j]), max(1, int(rng.integers(1, 2 + 2 * rest // max(len(room), 1)))))
        sizes[j] += add
        rest -= add
    out = np.concatenate((np.ones(n_single, np.int64), sizes))
    return out[rng.permutation(entries)]


def default_singles(H, entries):
    """about a third of the entries singletons, as far as H allows"""
    for n1 in range(min(entries, entries // 3 + 1), -1, -1):
        m = entries - n1
        if 2 * m <= H - n1 <= MAX_LIST * m:
            return n1
    for n1 in range(entries + 1):
        m = entries - n1
        if 2 * m <= H - n1 <= MAX_LIST * m:
            return n1
    raise AssertionError((H, entries))


def case(rng, name, shape, H, entries, n_single=None, s=16, kind="strong", sizes=None, read=None, **named):
    """a read of `shape` whose table lists give it H locations from `entries` found features"""
    read = read or new_read(rng, shape, s)
    assert entries <= len(read.real), (name, entries, len(read.real))
    if sizes is None:
        if kind == "singles":
            assert H == entries
            n_single = entries
        sizes = spread_sizes(rng, H, entries, default_singles(H, entries) if n_single is None else n_single)
    sizes = np.asarray(sizes, dtype=np.int64)
    assert len(sizes) == entries and int(sizes.sum()) == H, name
    slots = np.sort(rng.choice(read.real, entries, replace=False))
    lists = [np.zeros(0, np.uint64) for _ in read.feats]
    if kind == "singles":
        gw = singles(rng, entries)
        t, w = ol.split(gw)
        for j, tt, ww in zip(slots, t, w):
            lists[j] = np.array([(int(tt) << 32) | int(ww)], dtype=np.uint64)
    else:
        pool = _pool(rng, kind, max(int(sizes.max(initial=1)), min(max(H // 3, 12), 240)))
        for j, z in zip(slots, sizes):
            lists[j] = np.sort(rng.choice(pool, int(z), replace=False))
    return Case(name, read, lists, dict(named, H=H, entries=entries, kind=kind))


def lane_filler(rng, count, s=16, shape="single150"):
    """reads the lane finishes itself: 0 .. kLaneHits locations"""
    out = []
    for i in range(count):
        H = int(rng.integers(0, LANE_HITS + 1))
        r = new_read(rng, shape, s)
        if H == 0:                                                 # (none of its features is in the table)
            out.append(Case(f"lane filler {i}", r, [np.zeros(0, np.uint64)] * len(r.feats), dict(route="lane", H=0, entries=0)))
        else:
            out.append(case(rng, f"lane filler {i}", None, H, int(rng.integers(1, min(H, 20, len(r.real)) + 1)), s=s, read=r, route="lane"))
    return out


def handover_cases(rng, s=16, shape=None):
    """probe_cands_one's borders: H and the found features on both sides of kLaneHits, odd and even numbers of direct entries"""
    L = LANE_HITS
    shape = shape or ("single150" if s > 12 else "pair250")      # (at least kLaneHits + 2 features)
    c = []
    c.append(case(rng, "H kLaneHits, singletons only", shape, L, L, n_single=L, s=s, route="lane"))
    c.append(case(rng, "H kLaneHits, lists", shape, L, 5, s=s, route="lane"))
    c.append(case(rng, "H kLaneHits + 1, one list", shape, L + 1, L, n_single=L - 1, s=s, route="mid64", coop=True))
    c.append(case(rng, "H kLaneHits + 1, singletons: over", shape, L + 1, L + 1, n_single=L + 1, s=s, route="mid64", over=True))
    c.append(case(rng, "kLaneHits entries, no further one", shape, 60, L, s=s, route="mid64", coop=True))
    c.append(case(rng, "kLaneHits + 1 entries: over, odd", shape, 61, L + 1, s=s, route="mid64", over=True))
    c.append(case(rng, "kLaneHits + 2 entries: over, even", shape, 62, L + 2, s=s, route="mid64", over=True))
    full = new_read(rng, shape, s)
    c.append(case(rng, "every feature found", None, 64, len(full.real), s=s, read=full, route="mid64", over=True))
    c.append(case(rng, "one entry of 25", shape, L + 1, 1, s=s, route="mid64", coop=True))
    c.append(case(rng, "lists only, kLaneHits of them", shape, 2 * L, L, n_single=0, s=s, route="mid64", coop=True))
    return c


def class_cases(rng, s=16):
    """read_class's borders from both sides; named: the class on (compact, 8-byte) at the big_min the case names"""
    c = []

    def add(name, shape, H, entries, big_min, compact_route, wide_route, **kw):
        c.append(case(rng, name, shape, H, entries, s=s, big_min=big_min, routes={COMPACT: compact_route, WIDE8: wide_route}, **kw))
    BIG = 4096
    # ---- H at 64 / 65, 128 / 129, 256 / 257, 512 / 513, 1024 / 1025 with counting allowed (maxWin <= 8) and not (maxWin 9)
    for H, lo, hi in ((64, "mid64", "mid64"), (65, "hash256", "mid128"), (128, "hash256", "mid128"), (129, "hash256", "mid256"),
                      (256, "hash256", "mid256"), (257, "hash512", "wave"), (512, "hash512", "wave"), (513, "hash1024", "wave"),
                      (1024, "hash1024", "wave"), (1025, "wave", "wave")):
        add(f"H {H}, maxWin 8", "pair350", H, 40, BIG, lo, lo)
        add(f"H {H}, maxWin 9", "pair400", H, 40, BIG, hi, hi)
    add("H 200, maxWin 3", "single150", 200, 30, BIG, "hash256", "hash256")
    add("H 300, maxWin 11, 160 entries", "pair512", 300, 160, BIG, "wave", "wave")
    # ---- big_min 0 / 128 / 4096: H == bigMin against one more (and kMid64, below which nothing is filtered)
    add("big_min 0: H 64", "pair350", 64, 30, 0, "mid64", "mid64")
    add("big_min 0: H 65", "pair350", 65, 30, 0, "filter", "filter")
    add("big_min 0: H 65, maxWin 9", "pair400", 65, 30, 0, "filter", "mid128")
    add("big_min 128: H 128", "pair350", 128, 30, 128, "hash256", "hash256")
    add("big_min 128: H 129", "pair350", 129, 30, 128, "filter", "filter")
    add("big_min 128: H 129, maxWin 9", "pair400", 129, 30, 128, "filter", "mid256")
    add("big_min 4096: H 4096", "pair350", 4096, 60, 4096, "wave", "wave")
    add("big_min 4096: H 4097", "pair350", 4097, 60, 4096, "filter", "filter")
    add("big_min 128: H 2048", "pair350", 2048, 60, 128, "filter", "filter", second={COMPACT: False, WIDE8: False})
    add("big_min 128: H 2049", "pair350", 2049, 60, 128, "filter", "filter", second={COMPACT: True, WIDE8: False})
    return c


def mid_cases(rng, s=16):
    """mid_cands_kernel<4 / 8 / 16>: entries at 4 * G and one more, lists that fill G * kMidR slots and lists that leave padding,
    singletons only, lists only"""
    c = []
    for G, H, shape in ((4, 64, "pair400"), (8, 128, "pair400"), (16, 256, "pair400")):
        cls = {4: "mid64", 8: "mid128", 16: "mid256"}[G]
        lo = {4: LANE_HITS + 1, 8: 65, 16: 129}[G]
        for ent in (4 * G - 1, 4 * G, 4 * G + 1, 4 * G + 2 * G + 3):
            c.append(case(rng, f"mid<{G}>: {ent} entries, H {H}", shape, H, ent, s=s, route=cls))
            c.append(case(rng, f"mid<{G}>: {ent} entries, H {max(lo, ent)}", shape, max(lo, ent), ent, s=s, route=cls))
        c.append(case(rng, f"mid<{G}>: lists only", shape, H - 3, 2 * G, n_single=0, s=s, route=cls))
        c.append(case(rng, f"mid<{G}>: one list and singletons", shape, H - 1, 4 * G + 1, n_single=4 * G, s=s, route=cls))
    c.append(case(rng, "mid<4>: singletons only", "pair400", 64, 64, kind="singles", s=s, route="mid64"))
    c.append(case(rng, "mid<8>: singletons only", "pair400", 128, 128, kind="singles", s=s, route="mid128"))
    c.append(case(rng, "mid<16>: singletons only", "pair512", 160, 160, kind="singles", s=s, route="mid256"))
    c.append(case(rng, "mid<8>: one target", "pair400", 100, 30, kind="one_target", s=s, route="mid128"))
    c.append(case(rng, "mid<16>: one target", "pair400", 250, 30, kind="one_target", s=s, route="mid256"))
    c.append(case(rng, "mid<16>: targets without taxon", "pair400", 250, 30, kind="no_taxon", s=s, route="mid256"))
    return c


def full_list_cases(rng, s=16):
    """enough reads of each mid class to give every group of mid_cands_kernel's grid a read: 64 / G reads per wave, four waves per
    block, ceil(n / (256 / G)) blocks -- 65 reads of mid64, 33 of mid128, 17 of mid256 -> {class: cases}"""
    out = {}
    for G, cls, lo, hi in ((4, "mid64", LANE_HITS + 1, MID64), (8, "mid128", MID64 + 1, MID128), (16, "mid256", MID128 + 1, MID_MAX)):
        per_block = 4 * (64 // G)
        out[cls] = [case(rng, f"{cls} read {i}", "pair400", int(rng.integers(lo, hi + 1)), int(rng.integers(3, 25)), s=s, route=cls) for i in range(per_block + 1)]
    return out


def hash_cases(rng, s=16):
    """hash_cands_kernel<9 / 10 / 11>: per = ceil(H / 64) on both sides of every PER instance; entries at one wave-load and more;
    more distinct (target, window) pairs than one wave-load"""
    c = []
    pers = {"hash256": (2, 3, 4), "hash512": (5, 6, 7, 8), "hash1024": (10, 12, 14, 16)}
    for cls, ps in pers.items():
        for p in ps:
            for H in (64 * p, 64 * p + 1):
                want = read_class(H, 40, 8, 1 << 20, True)
                if want.startswith("hash"):
                    c.append(case(rng, f"{want}: per {-(-H // 64)}, H {H}", "pair350", H, 40, s=s, route=want))
    for ent in (63, 64, 65, 128):
        c.append(case(rng, f"hash256: {ent} entries", "pair391", 250, ent, s=s, route="hash256"))
        c.append(case(rng, f"hash1024: {ent} entries", "pair391", 1000, ent, s=s, route="hash1024"))
    c.append(case(rng, "hash256: singletons only", "pair391", 100, 100, kind="singles", s=s, route="hash256"))
    c.append(case(rng, "hash512: one target", "pair350", 400, 50, kind="one_target", s=s, route="hash512"))
    c.append(case(rng, "hash1024: one target", "pair350", 900, 50, kind="one_target", s=s, route="hash1024"))
    c.append(case(rng, "hash512: targets without taxon", "pair350", 400, 50, kind="no_taxon", s=s, route="hash512"))
    return c


def wave_cases(rng, s=16):
    """the wave kernels' own borders, met with the lane path off or K beyond kLaneK: kFuseCap (query_one<FUSE>), kLdsCap
    (sort_candidates_one: LDS against a segment in HBM)"""
    c = []
    for H in (FUSE_CAP, FUSE_CAP + 1, LDS_CAP, LDS_CAP + 1, 1500):
        c.append(case(rng, f"wave: H {H}", "pair400", H, 30, s=s, no_lane="wave"))
    c.append(case(rng, "wave: one target, H 600", "pair400", 600, 30, kind="one_target", s=s, no_lane="wave"))
    c.append(case(rng, "wave: singletons only", "pair400", 120, 120, kind="singles", s=s, no_lane="wave"))
    return c


def big_cases(rng, s=16):
    """8-byte store, the filtered path (big_min 0): entries at 64 / 65, the round shapes, kept lists at 512 / 513 and 1024 / 1025,
    fewer than K targets of two hits"""
    c = []

    def add(name, shape, H, entries, route, **kw):
        c.append(case(rng, name, shape, H, entries, s=s, big_min=0, routes={WIDE8: "filter"}, big=route, **kw))
    add("big: 64 entries", "pair350", 300, 64, "count", second=False)
    add("big: 65 entries", "pair350", 300, 65, "count", second=True)
    for kept, route in ((512, "count"), (513, "count2"), (1024, "count2"), (1025, "wave")):
        add(f"big: kept {kept}", "pair350", kept, 40, route, second=False)
        add(f"big: kept {kept}, second instance", "pair350", kept, 80, route, second=True)
    # rounds of 8 lanes up to r8 == kBigMaxRounds (32 lists of 64), of 16 beyond; of 16 up to r16 == kBigMaxRounds (64 lists of 64), of 64
    # beyond; more than kBigMaxRounds rounds of 64 (65 lists of 193 and more)
    add("big: r8 256", "pair350", 32 * 64, 32, "wave", sizes=[64] * 32, shape_=(256, 128, 3, 256))
    add("big: r8 257", "pair350", 32 * 64 + 2, 33, "wave", sizes=[64] * 32 + [2], shape_=(257, 129, 4, 129))
    add("big: r16 256", "pair350", 64 * 64, 64, "wave", sizes=[64] * 64, shape_=(512, 256, 4, 256))
    add("big: r16 257", "pair350", 64 * 64 + 2, 65, "wave", sizes=[64] * 64 + [2], shape_=(513, 257, 6, 65))
    add("big: R 256 at 64 lanes", "pair350", 64 * 254, 64, "wave", sizes=[254] * 64, shape_=(64 * 32, 64 * 16, 6, 256))
    add("big: R 257 at 64 lanes", "pair350", 64 * 254 + 2, 65, "wave", sizes=[254] * 64 + [2], shape_=(64 * 32 + 1, 64 * 16 + 1, 6, 257))
    add("big: one target (step D)", "pair350", 300, 40, "count", kind="one_target")
    add("big: one target, second instance", "pair350", 300, 70, "count", kind="one_target")
    add("big: targets without taxon", "pair350", 300, 40, "count", kind="no_taxon")
    add("big: one target, kept 800", "pair350", 800, 40, "count2", kind="one_target")
    add("big: one target, kept 1100", "pair350", 1100, 40, "wave", kind="one_target")
    return c


def tandem_cases(rng, s=16):
    """a read with a 20-mer repeated over the inside of one window (sketch_cases.tandem_read): the lane kernel leaves it to the wave
    kernel's sketching; on the compact store wave_rejoin_kernel applies filter_takes with the feature SLOTS as entries"""
    import sketch_cases
    out = []
    for H, side, kind in ((MID64, "sketch>wave", "strong"), (MID64 + 1, "sketch>filter", "strong"), (MID64, "sketch>wave", "one_target"),
                          (MID64 + 1, "sketch>filter", "one_target")):
        for _ in range(20):
            r = Read(sketch_cases.tandem_read(rng, KMER, WINLEN, STRIDE, 300, 1), b"", s)
            if r.dup and len(r.real) >= 12 and claim(rng, r):
                break
        assert r.dup and r.unique
        out.append(case(rng, f"tandem read, H {H}, {kind}", None, H, 12, s=s, read=r, kind=kind, big_min=0, routes={COMPACT: side, WIDE8: "sketch>wave"}))
    return out


def chunk_cases(rng, s=16):
    """long single reads (the chunk lanes): the feature slots are chunk_finish_kernel's entries -- 255 and 256 windows of 16 slots
    (4080, 4096) and, at sketch length 15, 273 windows (4095)"""
    out = []
    wins = (255, 256) if s == 16 else (273, 274) if s == 15 else ()
    for nw in wins:
        r = new_read(rng, ((nw - 1) * STRIDE + WINLEN, 0), s)
        assert r.windows == nw and r.chunked
        side = "chunk>filter" if nw * s <= REC_ENT_MAX else "chunk>wave"
        for kind in ("strong", "one_target"):
            rr = r if kind == "strong" else new_read(rng, ((nw - 1) * STRIDE + WINLEN, 0), s)
            out.append(case(rng, f"chunked read, {nw * s} feature slots, {kind}", None, 400, 60, s=s, read=rr, kind=kind, big_min=0,
                            routes={COMPACT: side, WIDE8: "chunk>wave"}))
    return out


def max_hits_cases(rng, s=16):
    """H == kMaxHitsPerQuery and one location more: 4 129 found features of a long single read (259 windows), lists of 254 -- about
    a million locations, 8 MB of table, each.  4 144 feature slots: beyond what the compact store's filtered path names
    (kRecEntMax), so both are the wave kernels' on either store; the longer one has no segment and no candidates."""
    out = []
    nw = -(-(-(-MAX_HITS // MAX_LIST) + 1) // s) + 1
    for extra in (0, 1):
        r = new_read(rng, ((nw - 1) * STRIDE + WINLEN, 0), s)
        ent = -(-(MAX_HITS + extra) // MAX_LIST)
        sizes = [MAX_LIST] * (ent - 1) + [MAX_HITS + extra - MAX_LIST * (ent - 1)]
        assert r.windows == nw and r.chunked and len(r.feats) > REC_ENT_MAX and ent <= len(r.real)
        pool = _pool(rng, "strong", 3000)
        slots = np.sort(rng.choice(r.real, ent, replace=False))
        lists = [np.zeros(0, np.uint64) for _ in r.feats]
        for j, z in zip(slots, sizes):
            lists[j] = np.sort(rng.choice(pool, z, replace=False))
        route = "too_many" if extra else "chunk>wave"
        out.append(Case(f"kMaxHitsPerQuery + {extra}", r, lists, dict(H=MAX_HITS + extra, entries=ent, big_min=0, routes={COMPACT: route, WIDE8: route})))
    return out


def first_slots(cases):
    """fbase of every read of a batch: the feature slots in front of it (put_entry's pairs need it even)"""
    return np.concatenate(([0], np.cumsum([len(c.read.feats) for c in cases])))[:-1]


def named_route(c: Case, store: str):
    """the route a case was built for on this store (None: the builder names none)"""
    if "routes" in c.named:
        return c.named["routes"].get(store)
    return c.named.get("route")


def case_big_min(c: Case) -> int:
    return c.named.get("big_min", NO_FILTER)


# ---- the device side ----------------------------------------------------------------------------------------------------------
def table_of(cases):
    """(keys, sizes, vals{window, target}) of every found feature of the cases; no two reads share a feature"""
    seen = {}
    keys, sizes, vals = [], [], []
    for c in cases:
        assert len(set(c.read.feats[c.read.real].tolist())) == len(c.read.real), ("a hash twice in one read", c.name)
        for f in c.read.feats[c.read.real].tolist():
            assert seen.setdefault(f, c.name) == c.name, ("two reads share a feature", c.name, seen[f])
        for f, x in zip(c.read.feats.tolist(), c.lists):
            if len(x):
                keys.append(f)
                sizes.append(len(x))
                vals.append(np.stack(((x & np.uint64(0xFFFFFFFF)).astype(np.uint32), (x >> np.uint64(32)).astype(np.uint32)), axis=1))
    vals = np.ascontiguousarray(np.concatenate(vals), dtype=np.uint32) if vals else np.zeros((0, 2), np.uint32)
    assert np.all(vals[:, 1] < NT) and np.all(vals[:, 0] < WINDOWS[vals[:, 1]])                 # every location is a window of its target
    return np.array(keys, dtype=np.uint32), np.array(sizes, dtype=np.uint8), vals


def context(cases, store: str, K: int, s: int = 16, copy_allhits: int = 0, max_queries: int = 1 << 10, max_chars: int = 1 << 20):
    """a context whose table holds the cases' lists -> api.Database"""
    from metacache_amd import api
    L = api.lib()
    cfg = api.default_config(target_id_bytes=4, max_candidates=K, sketchlen=s, num_slots=1, slot_max_queries=max_queries,
                             slot_max_chars=max_chars, copy_allhits=copy_allhits)
    assert (cfg.kmerlen, cfg.winlen, cfg.winstride) == (KMER, WINLEN, STRIDE)
    h = C.c_void_p()
    assert L.mc_create(C.byref(cfg), C.byref(h)) == 0, L.mc_last_error(None)
    db = api.Database.from_handle(h.value, cfg)
    try:
        if store == COMPACT:
            db.load_target_windows(WINDOWS)
        else:
            db.set_tuning("compact_locations", 0)
        keys, sizes, vals = table_of(cases)
        db._check(L.mc_load_begin(db.h, 0, len(keys), len(vals)))
        db._check(L.mc_load_batch(db.h, 0, keys.ctypes.data, sizes.ctypes.data, vals.ctypes.data, len(keys)))
        db._check(L.mc_load_end(db.h, 0))
        lay = db.table_layout()
        assert lay["location_bytes"] == (4 if store == COMPACT else 8) and not lay["direct_index"], lay
        assert store != COMPACT or lay["window_gap"] == GAP, lay
        lin = np.zeros((NT, 21), dtype=np.uint32)
        lin[:, TAX_RANK] = TAX
        db.set_lineages(lin)
        db.refresh_info()
        assert (db.k, db.s, db.w, db.stride) == (KMER, s, WINLEN, STRIDE)
        return db
    except Exception:
        db.close()
        raise


TIMERS = tuple(TIMER_OF.values()) + ("big_filter", "big_filter_2", "big_count", "big_count_2", "gw_filter_count", "gw_filter", "sort_candidates",
                                     "query_wave", "chunk_probe", "probe_cands", "sketch_probe")


def expected_timers(routes, store, seconds, lane_path=True, gw_fuse=1):
    """{timer: launched} as the host's rules give it for a batch of these routes (query_pipe.cpp: run_mid_and_hash, tail_plan)"""
    compact = store == COMPACT
    has = lambda *r: any(x in routes for x in r)
    want = {t: False for t in TIMERS if t not in ("chunk_probe", "probe_cands", "sketch_probe")}
    if not lane_path:
        want["sort_candidates"] = want["query_wave"] = True
        return want
    for cls, timer in TIMER_OF.items():
        want[timer] = has(cls)
    sketch = has("sketch>filter", "sketch>wave")
    filt = has("filter", "chunk>filter") or (compact and sketch)                    # (waveFirst: the filtered path runs for what may rejoin)
    if compact:
        want["gw_filter_count" if gw_fuse else "gw_filter"] = filt
    else:
        want["big_filter"] = want["big_count"] = want["big_count_2"] = filt
        want["big_filter_2"] = filt and seconds > 0
    wave = filt or sketch or has("wave", "chunk>wave", "too_many")
    want["sort_candidates"] = want["query_wave"] = wave
    return want


def pack_batch(cases):
    """the batch as mc_query_device takes it: every sequence at a multiple of four characters, qinfo rows {first, length, first of the
    mate, its length}, maxWindowsInRange per read -> (characters with 64 readable bytes behind them, qinfo, max_win, characters)"""
    parts, info, at = [], np.zeros((len(cases), 4), dtype=np.uint32), 0
    for q, c in enumerate(cases):
        for j, seq in enumerate((c.read.seq1, c.read.seq2)):
            info[q, 2 * j], info[q, 2 * j + 1] = at, len(seq)
            pad = -len(seq) % 4
            parts.append(np.frombuffer(seq + b"N" * pad, dtype=np.uint8))
            at += len(seq) + pad
    seq = np.concatenate(parts + [np.full(64, ord("N"), dtype=np.uint8)])
    return seq, info, np.array([c.max_win for c in cases], dtype=np.uint32), at


def run_device(db, cases, K, lowest):
    """mc_query_device on the first pipe (the call mc_last_batch_stats speaks of) -> (cands[n, K], qstat[n])"""
    import torch
    from metacache_amd import api
    seq, info, mw, chars = pack_batch(cases)
    dev = torch.device("cuda", 0)
    dseq, dq, dmw = (torch.from_numpy(a.view(np.uint8)).to(dev) for a in (seq, info.reshape(-1), mw))
    n = len(cases)
    res = db.query_device(dseq.data_ptr(), dq.data_ptr(), n, chars, max_win_ptr=dmw.data_ptr(), lowest=lowest)
    db.synchronize()
    cands = np.zeros((n, K), dtype=api.cand_dtype)
    qstat = np.zeros(n, dtype=api.qstat_dtype)
    db.copy_results(cands.ctypes.data, res.cands, cands.nbytes, to_host=True)
    db.copy_results(qstat.ctypes.data, res.hit_counts, qstat.nbytes, to_host=True)
    db.synchronize()
    return cands, qstat


def check(db, cases, K, lowest, store, big_min=BIG_MIN_DEFAULT, lane_path=True, tuning=None, allhits=False):
    """ONE db.query of the cases in this order (the host's slots), and the same batch through mc_query_device, whose statistics
    mc_last_batch_stats reports; everything against the model -> {route: reads}"""
    tax = lowest != 0
    assert K == db.cfg.max_candidates and len(cases) <= db.cfg.slot_max_queries
    assert sum((len(c.read.seq1) + 3) // 4 * 4 + (len(c.read.seq2) + 3) // 4 * 4 for c in cases) <= db.cfg.slot_max_chars
    lane = lane_path and K <= LANE_K and not allhits
    tuning = dict(tuning or {})
    tuning.update(big_min=big_min, lane_path=int(lane_path))
    for c in cases:
        assert db.max_windows_in_range(len(c.read.seq1), len(c.read.seq2)) == c.max_win, c.name
    for name, v in tuning.items():
        db.set_tuning(name, v)
    from metacache_amd import api
    db.timing(True)
    try:
        db.timing_reset()
        refused = None
        try:
            cands, counts, hits = db.query([c.read.seq1 for c in cases], [c.read.seq2 for c in cases], lowest=lowest)
        except api.McError as e:                                   # mc_batch_wait: a read beyond kMaxHitsPerQuery fails its whole slot
            if "more than 2^20-1 location hits" not in str(e):
                raise
            refused, cands, counts, hits = str(e), None, None, None
            db._check(api.lib().mc_batch_clear(db.h, 0))
        assert (refused is not None) == any(c.H > MAX_HITS for c in cases), refused
        ran = {"db.query": {t: db.timing_get(t)[1] for t in TIMERS}}
        dcands = qstat = stats = None
        if not allhits:                                            # (a context that copies the lists takes the wave kernels in its slots only)
            db.timing_reset()
            dcands, qstat = run_device(db, cases, K, lowest)
            stats = db.last_batch_stats()
            ran["mc_query_device"] = {t: db.timing_get(t)[1] for t in TIMERS}
    except api.McError as e:                                       # a device error: nothing more is started on that device
        import pytest
        if "error -2:" in str(e):                                  # MC_ERR_HIP
            pytest.exit(f"device error in a batch of {len(cases)} reads ({store}, K {K}, big_min {big_min}, {tuning}): {e}", returncode=3)
        raise
    finally:
        db.timing(False)
        for name, v in (("big_min", BIG_MIN_DEFAULT), ("lane_path", 1), ("quad_lookup", -1), ("lane_fusion", -1)):
            db.set_tuning(name, v)
    bad, reached = [], {}
    seconds = 0
    for q, c in enumerate(cases):
        route = route_of(c, store, big_min, lane)
        if route == "filter" and store == WIDE8:
            seconds += filter_second(c.H, c.entries, False)
            route = "filter>" + big_route(c)
        reached[route] = reached.get(route, 0) + 1
        exp = c.expected(K, tax)
        for what, rows in (("db.query", cands), ("mc_query_device", dcands)):
            if rows is None:
                continue
            if exp is None:
                if (rows[q]["hits"] != 0).any():
                    bad.append((q, c.name, route, what, "candidates of a read without an answer", rows[q].tolist()))
            elif not same_candidates(rows[q], exp):
                bad.append((q, c.name, route, what, rows[q].tolist(), exp.tolist()))
        if counts is not None and int(counts[q]) != c.H:
            bad.append((q, c.name, route, "count", int(counts[q]), c.H))
        if qstat is not None and (int(qstat[q]["hits"]), int(qstat[q]["nfeat"]), int(qstat[q]["nfound"])) != (c.H, c.nfeat, c.entries):
            bad.append((q, c.name, route, "locations, features probed, features found", qstat[q].tolist(), (c.H, c.nfeat, c.entries)))
        if allhits and not np.array_equal(_as_u64(hits[q]), c.locs):
            bad.append((q, c.name, route, "allhits", len(hits[q]), c.H))
    if stats is not None:
        want = dict(windows=sum(c.read.windows for c in cases), features=sum(c.nfeat for c in cases), locations=sum(c.H for c in cases),
                    found=sum(c.entries for c in cases))
        got = {k: stats[k] for k in want}
        if got != want:
            bad.append(("last_batch_stats", got, want))
        if lane and store == WIDE8:
            nfilter = sum(v for r, v in reached.items() if r.startswith("filter"))
            if (stats["filtered_reads"], stats["filter_second_kernel"]) != (nfilter, seconds):
                bad.append(("filtered reads, second instance", stats["filtered_reads"], stats["filter_second_kernel"], nfilter, seconds))
    plain = {r.split(">")[0] if r.startswith("filter>") else r for r in reached}
    for call, counted in ran.items():
        for t, w in expected_timers(plain, store, seconds, lane, tuning.get("gw_fuse", 1)).items():
            if bool(counted[t]) != w:
                bad.append(("timer", call, t, counted[t], w))
    assert not bad, (store, K, lowest, big_min, tuning, len(cases), len(bad), bad[:6])
    return reached


def _as_u64(h):
    """api.loc_dtype rows -> (target << 32 | window)"""
    h = np.asarray(h)
    return (h["tgt"].astype(np.uint64) << np.uint64(32)) | h["win"].astype(np.uint64)


# the literal rows the CPU test pins read_class() against: (H, entries, maxWin, bigMin, compact) -> class number of read_class.h
# (0 kListMid64, 1 kListMid128, 2 kListMid256, 3 kListHash512, 4 kListHash1024, 5 kListHash256, 6 kClassWave, 7 kClassFilter)
CLASS_ROWS = [
    ((25, 25, 3, 128, True), 0), ((64, 30, 8, 0, True), 0), ((65, 30, 8, 0, True), 7), ((65, 30, 8, 0, False), 7), ((65, 30, 9, 0, False), 1),
    ((65, 30, 9, 0, True), 7), ((65, 30, 1024, 0, True), 7), ((65, 30, 1025, 0, True), 1), ((65, 30, 8, 128, True), 5), ((128, 30, 8, 128, False), 5),
    ((129, 30, 8, 128, False), 7), ((129, 30, 9, 128, False), 2), ((129, 30, 9, 128, True), 7), ((128, 30, 9, 128, True), 1), ((128, 257, 8, 128, True), 1),
    ((256, 256, 8, 4096, True), 5), ((256, 257, 8, 4096, True), 2), ((256, 30, 9, 4096, False), 2), ((257, 30, 9, 4096, False), 6), ((257, 30, 8, 4096, False), 3),
    ((512, 30, 8, 4096, True), 3), ((513, 30, 8, 4096, True), 4), ((1024, 30, 8, 4096, True), 4), ((1025, 30, 8, 4096, True), 6), ((4096, 60, 8, 4096, True), 6),
    ((4097, 60, 8, 4096, True), 7), ((4097, 60, 8, 4096, False), 7), ((4097, 60, 9, 4096, False), 6), ((300, 192, 8, 0, False), 7), ((300, 193, 8, 0, False), 3),
    ((300, 4095, 8, 0, True), 7), ((300, 4096, 8, 0, True), 6), ((1048575, 100, 8, 0, True), 7), ((1048576, 100, 8, 0, True), 6), ((64, 64, 11, 0, True), 0),
]
