"""TEST INFRASTRUCTURE: chosen location lists for the database builder (csrc/builder.hip), a plain model of what the builder must make of
them, and the calls and comparisons of tests/test_gpu_builder_lists.py.  tests/test_builder_lists_cpu.py proves, from the model alone,
that every case sits on the border it is named for.

The lists go in through the two modify-mode entry points -- mc_build_add_existing_target, mc_build_add_locations -- which take any
(key, size, packed values) batches without sketching; from there mc_build_finish, mc_build_remove_ambiguous, mc_build_write* and
mc_build_finish_shards run the real device stages (stable sort, run count, cap, compaction, ambiguity, hand-over to the table, file batches).

THE MODEL (written from the contract in include/metacache_amd.h, not from the kernels):
  * a feature's locations are all its pairs in ARRIVAL order: batch after batch, entry after entry (the same key may stand in several
    batches and several times in one), then whatever real targets sketch, target after target, window after window;
  * the first maxLocs of them are kept, maxLocs = min(max_locations_per_feature or 254, 254);
  * shard i of n keeps key k iff key_owner(k, n) == i (table_rules.h; mirrored below with the constants read from the header);
  * key 0xFFFFFFFF is never stored;
  * remove_overpopulated and maxLocs > 1: a feature whose kept list is longer than maxLocs - 1 is absent from the written file and empty
    ("dead") in the loaded table -- the builder itself still HOLDS it: mc_build_counts and mc_build_remove_ambiguous see it (the rule is
    applied by mc_build_write_add and by the table's load filter, builder.hip);
  * ambiguity: over the kept list, more than max(maxAmbig, 1) different anc[target] -> the feature goes; ancestor 0 is one taxon.

WHAT THE MODEL AND THESE CASES LEAVE OPEN, and why:
  * mc_build_write_add's host slice of 2^24 keys: a second slice needs about 200 MB of pairs and seconds of sorting per test;
  * more than 2^32 (feature, location) pairs in one builder (refused by mc_build_finish): 48 GB of pairs;
  * count_runs_kernel's grid-stride loop, which begins beyond 65536 blocks = 2^24 pairs: the same size;
  * the streaming calls (mc_build_table_begin/_add/_end, mc_build_write_begin/_add/_end) are reached only through
    mc_build_finish_shards and mc_build_write_shards, which are those three in a row;
  * device-resident targets (mc_build_add_target_device) and the sketchers: tests/test_gpu_builder_sketchers.py."""
import ctypes as C
import os
import re

import numpy as np

from table_model import Table, check_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metacache_amd", "csrc")

MC_ERR_INVALID, MC_ERR_UNSUPPORTED, MC_ERR_STATE = -1, -5, -6
NO_KEY = 0xFFFFFFFF
MAX_LIST = 254                                    # the ceiling of a stored list (bucket_size_type u8, host_hashmap.hpp)
FILE_BATCH = 1 << 20                              # keys per batch of the .cache file (mc_db_writer::hdr[2])
TABLE_CHUNK = 1 << 22                             # keys per hand-over chunk of mc_build_table_add
SMALL_SLOTS = dict(num_slots=1, slot_max_queries=64, slot_max_chars=1 << 16)      # (no queries here: small slots)


# ---- the key-shard rule, mirrored ---------------------------------------------------------------------------------------------------
def _rule_constants():
    """mix32's shifts and multipliers and key_owner's xor constant, read from table_rules.h"""
    txt = open(os.path.join(CSRC, "table_rules.h")).read()
    m = re.search(r"uint32_t mix32\(uint32_t x\)\s*\{\s*x \^= x >> (\d+); x \*= (0x[0-9a-fA-F]+)u; x \^= x >> (\d+); x \*= (0x[0-9a-fA-F]+)u; x \^= x >> (\d+);", txt)
    o = re.search(r"mix32\(key \^ (0x[0-9a-fA-F]+)u\) \* shards\) >> 32", txt)
    assert m and o
    return [int(m.group(i), 0) for i in range(1, 6)], int(o.group(1), 0)


(SH1, MUL1, SH2, MUL2, SH3), OWNER_XOR = _rule_constants()


def mix32(x):
    x = np.asarray(x, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    x = x ^ (x >> np.uint64(SH1)); x = (x * np.uint64(MUL1)) & np.uint64(0xFFFFFFFF)
    x = x ^ (x >> np.uint64(SH2)); x = (x * np.uint64(MUL2)) & np.uint64(0xFFFFFFFF)
    return x ^ (x >> np.uint64(SH3))


def key_owner(keys, shards):
    keys = np.asarray(keys, dtype=np.uint64)
    if shards <= 1:
        return np.zeros(keys.shape, dtype=np.uint32)
    return ((mix32(keys ^ np.uint64(OWNER_XOR)) * np.uint64(shards)) >> np.uint64(32)).astype(np.uint32)


# rows computed once by a host program that includes table_rules.h: (key, owner of 1, 2, 3, 7, 64 shards)
OWNER_ROWS = [
    (0x00000000, 0, 1, 1, 4, 36), (0x00000001, 0, 0, 0, 1, 13), (0x00000002, 0, 1, 2, 4, 45), (0x7FFFFFFF, 0, 0, 1, 2, 21),
    (0x80000000, 0, 1, 2, 5, 47), (0xFFFFFFFE, 0, 0, 0, 1, 13), (0xFFFFFFFF, 0, 0, 0, 1, 14), (0x075BCD15, 0, 1, 2, 5, 45),
    (0x9E3779B9, 0, 0, 0, 0, 0), (0x00010000, 0, 1, 2, 6, 63), (0x01010101, 0, 1, 1, 4, 36), (0xDEADBEEF, 0, 1, 2, 4, 45),
]
OWNER_SHARDS = (1, 2, 3, 7, 64)


# ---- a case -------------------------------------------------------------------------------------------------------------------------
class Case:
    """windows[t] of the existing targets; batches = [(keys u32[n], sizes u8[n], vals u32[sum sizes, 2] = {win, tgt})] as
    mc_build_add_locations takes them; real = sequences sketched afterwards (their targets follow the existing ones); the builder's
    max_locations_per_feature, remove_overpopulated, target_id_bytes; pack = target bytes of the packed values handed in;
    classes = {name: keys} for the proofs of tests/test_builder_lists_cpu.py; anc = ancestor of every target (ambiguity cases)"""

    def __init__(self, name, windows, batches, max_locs=0, rm_over=0, tb=4, pack=None, real=(), classes=None, anc=None):
        self.name = name
        self.windows = np.asarray(windows, dtype=np.uint64)
        self.batches = [(np.ascontiguousarray(k, dtype=np.uint32), np.ascontiguousarray(s, dtype=np.uint8),
                         np.ascontiguousarray(v, dtype=np.uint32).reshape(-1, 2)) for k, s, v in batches]
        for k, s, v in self.batches:
            assert len(k) == len(s) and int(s.astype(np.int64).sum()) == len(v)
        self.max_locs, self.rm_over, self.tb, self.pack = max_locs, rm_over, tb, pack or tb
        self.real = list(real)
        self.classes = classes or {}
        self.anc = None if anc is None else np.asarray(anc, dtype=np.uint32)
        self._pairs = None

    @property
    def cap(self):
        return min(self.max_locs or MAX_LIST, MAX_LIST)

    @property
    def rule_on(self):
        """the build-time overpopulation rule: off with a cap of 1 (mc_build_begin: buckets of one location always stay)"""
        return bool(self.rm_over) and self.cap > 1

    @property
    def n_targets(self):
        return len(self.windows) + len(self.real)

    def pairs(self):
        """every (key, (tgt << 32) | win) in arrival order"""
        if self._pairs is None:
            ks = [np.repeat(k, s) for k, s, _ in self.batches]
            vs = [(v[:, 1].astype(np.uint64) << np.uint64(32)) | v[:, 0].astype(np.uint64) for _, _, v in self.batches]
            for i, g in enumerate(self.real):
                import cpuref
                feats, counts = cpuref.oracle().sketch(bytes(g), 16, 16, 127, 112)
                t = np.uint64(len(self.windows) + i)
                for w in range(len(counts)):
                    ks.append(feats[w, :counts[w]].astype(np.uint32))
                    vs.append(np.full(int(counts[w]), (t << np.uint64(32)) | np.uint64(w), dtype=np.uint64))
            self._pairs = (np.concatenate(ks) if ks else np.zeros(0, np.uint32), np.concatenate(vs) if vs else np.zeros(0, np.uint64))
        return self._pairs


def _table(keys, sizes, vals64):
    vals64 = np.asarray(vals64, dtype=np.uint64)
    return Table(keys, sizes, np.stack([vals64 & np.uint64(0xFFFFFFFF), vals64 >> np.uint64(32)], axis=1))


def vals64(table):
    return (table.vals[:, 1].astype(np.uint64) << np.uint64(32)) | table.vals[:, 0].astype(np.uint64)


def held(case, shard=0, shards=1):
    """what builder `shard` of `shards` holds after mc_build_finish: keys ascending, the first `cap` locations of each in arrival order.
    .arrived[i] = locations that arrived for key i, .run_start[i] = index of its first pair among the builder's pairs ordered by key"""
    k, v = case.pairs()
    keep = k != NO_KEY
    nokey = int((~keep & (key_owner(k, shards) == shard)).sum())
    if shards > 1:
        keep &= key_owner(k, shards) == shard
    k, v = k[keep], v[keep]
    order = np.argsort(k, kind="stable")                                    # groups by key; arrival order stays inside a key
    ks, vs = k[order], v[order]
    start = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]])) if len(ks) else np.zeros(0, np.int64)
    counts = np.diff(np.concatenate([start, [len(ks)]]))
    rank = np.arange(len(ks)) - np.repeat(start, counts)
    t = _table(ks[start], np.minimum(counts, case.cap), vs[rank < case.cap])
    t.arrived, t.run_start, t.pairs, t.nokey_pairs = counts, start, len(ks) + nokey, nokey
    return t


def whole(tables):
    """the tables of the shards of one set as one table, keys ascending"""
    keys = np.concatenate([t.keys for t in tables])
    order = np.argsort(keys, kind="stable")
    sizes = np.concatenate([t.sizes for t in tables])[order]
    first = np.concatenate([t.first + off for t, off in zip(tables, np.cumsum([0] + [len(t.vals) for t in tables])[:-1])])[order]
    vals = np.concatenate([t.vals for t in tables])
    n = sizes.astype(np.int64)
    flat = np.repeat(first, n) + (np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n))
    return Table(keys[order], sizes, vals[flat.astype(np.int64)])


def subset(table, keep):
    keep = np.asarray(keep, dtype=bool)
    n = table.sizes.astype(np.int64)
    return Table(table.keys[keep], table.sizes[keep], table.vals[np.repeat(keep, n)])


def taxa_of(table, anc):
    """number of different ancestors on every kept list"""
    a = np.asarray(anc)[table.vals[:, 1]]
    return np.array([len(set(a[f:f + s].tolist())) for f, s in zip(table.first.tolist(), table.sizes.tolist())], dtype=np.int64)


def without_ambiguous(table, anc, max_ambig):
    """host_hashmap.hpp:499-540 as restated in test_remove_ambiguous_features: more than max(max_ambig, 1) taxa -> gone"""
    return subset(table, taxa_of(table, anc) <= max(max_ambig, 1))


def written(table, case):
    """what the file and a table opened from it hold: with the overpopulation rule, only lists of at most cap - 1"""
    return subset(table, table.sizes <= case.cap - 1) if case.rule_on else table


# ---- generators ---------------------------------------------------------------------------------------------------------------------
SMALL_WINDOWS = [300, 40, 1000, 7, 300]           # five existing targets; 1647 different locations


def spread_keys(rng, n, used, shards=3):
    """n new keys whose owners of `shards` go round 0, 1, 2, 0, ...: every shard owns one in three of every class"""
    out = []
    while len(out) < n:
        k = int(rng.integers(2, NO_KEY - 1))
        if k not in used and int(key_owner(k, shards)) == len(out) % shards:
            used.add(k); out.append(k)
    return out


def some_locations(rng, windows, n, order):
    """n different locations of the targets, ascending / descending / shuffled in (target, window) order -> [n, 2] = {win, tgt}"""
    windows = np.asarray(windows, dtype=np.int64)
    base = np.concatenate([[0], np.cumsum(windows)])
    g = np.sort(rng.choice(int(base[-1]), size=n, replace=False))
    tgt = np.searchsorted(base, g, side="right") - 1
    locs = np.stack([g - base[tgt], tgt], axis=1)
    if order == "desc":
        locs = locs[::-1]
    elif order == "shuffled":
        locs = locs[rng.permutation(n)]
        if n > 1 and np.all(np.diff((locs[:, 1] << 32) | locs[:, 0]) > 0):
            locs = locs[::-1]
    return locs.astype(np.uint32)


def chunks_of(rng, n, first=None):
    """a list of n locations as entry sizes 0 .. 255"""
    out = [] if first is None else [first]
    left = n - sum(out)
    while left > 0:
        c = min(int(rng.choice([0, 1, 1, 2, 3, 5, 17, 100, 255])), left)
        out.append(c); left -= c
    if rng.random() < 0.3:
        out.append(0)
    return out


def batches_of(rng, lists, nbatches=4):
    """lists = [(key, locs[n, 2], entry sizes)] -> batches: the entries of a key keep their order, go to batches that never go back, and
    stand behind each other inside a batch as they come; keys mix freely otherwise"""
    per = [[] for _ in range(nbatches)]
    for key, locs, sizes in lists:
        assert sum(sizes) == len(locs) and max(sizes, default=0) <= 255
        where = np.sort(rng.integers(0, nbatches, size=len(sizes)))
        at, seen = 0, {}
        for b, s in zip(where.tolist(), sizes):
            seen[b] = seen.get(b, 0) + 1
            per[b].append((seen[b], float(rng.random()), key, locs[at:at + s]))
            at += s
    out = []
    for entries in per:
        entries.sort(key=lambda e: (e[0], e[1]))
        keys = [e[2] for e in entries]
        sizes = [len(e[3]) for e in entries]
        vals = np.concatenate([e[3] for e in entries]) if entries else np.zeros((0, 2), np.uint32)
        out.append((keys, sizes, vals.reshape(-1, 2)))
    return out


ORDERS = ("asc", "desc", "shuffled")
PER_CLASS = 6                                      # keys of every length class: two for each of three shards


def cap_case(m, rm_over=0, tb=4, pack=None, seed=1):
    """item 1 (and 7, 8): for the cap M that max_locations_per_feature = m means, lists of 1, M - 2, M - 1, M, M + 1 and 3M + 1 locations,
    one list that is a single entry of 255, keys whose entries are all empty; long lists come in several entries over several batches,
    in ascending, descending and shuffled (target, window) order"""
    rng = np.random.default_rng(1000 * seed + m)
    M = min(m or MAX_LIST, MAX_LIST)
    lengths = {"one": 1, "m-2": M - 2, "m-1": M - 1, "m": M, "m+1": M + 1, "3m+1": 3 * M + 1, "entry255": 255}
    used, lists, classes = set(), [], {}
    for cname, n in lengths.items():
        if n < 1:
            continue
        classes[cname] = spread_keys(rng, PER_CLASS, used)
        for j, key in enumerate(classes[cname]):
            locs = some_locations(rng, SMALL_WINDOWS, n, ORDERS[(j // 3 + j) % 3])
            if cname == "entry255":
                sizes = [255]
            else:
                sizes = chunks_of(rng, n, first=255 if n >= 255 and j == 0 else None)
            lists.append((key, locs, sizes))
    classes["empty"] = spread_keys(rng, 3, used)
    lists += [(key, np.zeros((0, 2), np.uint32), [0, 0]) for key in classes["empty"]]
    return Case(f"cap{m}" + ("_rm" if rm_over else "") + f"_tb{tb}", SMALL_WINDOWS, batches_of(rng, lists), max_locs=m, rm_over=rm_over, tb=tb, pack=pack,
                classes=classes)


EDGE_KEYS = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE]
BIT_BASE = 0x5A3C9617


def key_case():
    """item 2: the smallest and largest keys, both sides of the sign bit, pairs of keys one bit apart in every byte (a radix pass that
    is skipped or reads the wrong digit merges or misorders them), and key 0xFFFFFFFF with a list"""
    rng = np.random.default_rng(22)
    pairs = [BIT_BASE] + [BIT_BASE ^ (1 << b) for b in (0, 7, 8, 15, 16, 23, 24, 31)]
    keys = EDGE_KEYS + pairs
    lists = [(k, some_locations(rng, SMALL_WINDOWS, n, ORDERS[i % 3]), chunks_of(rng, n)) for i, k in enumerate(keys) for n in [1 + i % 5]]
    lists.append((NO_KEY, some_locations(rng, SMALL_WINDOWS, 3, "asc"), [2, 1]))
    return Case("keys", SMALL_WINDOWS, batches_of(rng, lists, 3), classes={"edge": EDGE_KEYS, "bits": pairs, "nokey": [NO_KEY]})


def nokey_only_case():
    rng = np.random.default_rng(23)
    return Case("nokey_only", SMALL_WINDOWS, batches_of(rng, [(NO_KEY, some_locations(rng, SMALL_WINDOWS, 5, "desc"), [1, 0, 4])], 2))


def no_pairs_case():
    return Case("no_pairs", SMALL_WINDOWS, [])


def runs_case(nkeys, every=1, seed=3):
    """item 3: nkeys distinct keys with lists of `every` locations (every = 0: lengths 1, 1, 1, 2, 3 mixed), one pair per entry, shuffled"""
    rng = np.random.default_rng(seed * 100000 + nkeys)
    keys = np.unique(rng.integers(0, NO_KEY, size=nkeys + 64, dtype=np.uint64).astype(np.uint32))
    keys = rng.permutation(keys)[:nkeys]
    n = np.full(nkeys, every) if every else rng.choice([1, 1, 1, 2, 3], size=nkeys)
    k = rng.permutation(np.repeat(keys, n))
    g = rng.integers(0, sum(SMALL_WINDOWS), size=len(k))
    base = np.concatenate([[0], np.cumsum(SMALL_WINDOWS)])
    tgt = np.searchsorted(base, g, side="right") - 1
    vals = np.stack([g - base[tgt], tgt], axis=1)
    half = len(k) // 2
    one = np.ones(len(k), np.uint8)
    return Case(f"runs{nkeys}_{every}", SMALL_WINDOWS, [(k[:half], one[:half], vals[:half]), (k[half:], one[half:], vals[half:])])


def run_edge_case():
    """item 3: after sorting, runs begin at pair index 255, 256 and 257 -- count_runs_kernel's keys[i - 1] on both sides of a block edge"""
    rng = np.random.default_rng(31)
    lists = [(10, some_locations(rng, SMALL_WINDOWS, 255, "shuffled"), [100, 155]), (11, some_locations(rng, SMALL_WINDOWS, 1, "asc"), [1]),
             (12, some_locations(rng, SMALL_WINDOWS, 1, "asc"), [1]), (13, some_locations(rng, SMALL_WINDOWS, 2, "desc"), [1, 1])]
    return Case("run_edge", SMALL_WINDOWS, batches_of(rng, lists, 3))


def id_case(tb):
    """item 5: the largest target ids of the packing, first and last windows, and (tb = 4) a target of 2^24 + 10 windows with a singleton
    and a list at window 2^24 + 5, where the table's direct index cannot hold the location"""
    rng = np.random.default_rng(50 + tb)
    if tb == 2:
        windows = np.full(0xFFFF, 4, dtype=np.uint64)                       # 65535 targets: ids 0 .. 0xFFFE
        tgts = [0, 255, 256, 0xFFFE]
    else:
        windows = np.full(65538, 4, dtype=np.uint64)
        windows[65536] = (1 << 24) + 10
        tgts = [0, 65535, 65536, 65537]
    ends = np.array([[w, t] for t in tgts for w in (0, int(windows[t]) - 1)], dtype=np.uint32)
    lists = [(100 + i, ends[i:i + 1], [1]) for i in range(len(ends))]      # singletons: inline payloads
    lists.append((200, ends, [3, len(ends) - 3]))                            # one list through all of them, ascending
    lists.append((201, ends[::-1], [len(ends)]))                             # and descending
    classes = {"ends": [100 + i for i in range(len(ends))] + [200, 201]}
    if tb == 4:
        far = np.array([[(1 << 24) + 5, 65536]], dtype=np.uint32)
        lists.append((300, far, [1]))
        lists.append((301, np.concatenate([ends[:2], far, ends[-2:]]), [2, 3]))
        classes["far"] = [300, 301]
    return Case(f"ids_tb{tb}", windows, batches_of(rng, lists, 2), tb=tb, classes=classes)


def random_genome(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].copy()


def existing_case(m=7):
    """item 6: two real targets sketched behind existing lists of m - 2, m - 1 and m locations on features of their own; the features are of a
    stretch that stands twice in the first genome and once in the second, so three sketched locations follow each existing list and
    the cap cuts among them; untouched features of both genomes beside them"""
    import cpuref
    rng = np.random.default_rng(60)
    g = [random_genome(rng, 2100), random_genome(rng, 1900)]
    g[0][1456:1756] = g[0][784:1084]               # windows 13, 14 of the first = its windows 7, 8 = windows 3, 4 of the second:
    g[1][336:636] = g[0][784:1084]                 # their features are sketched three times
    feats, counts = cpuref.oracle().sketch(bytes(g[0]), 16, 16, 127, 112)
    assert np.array_equal(feats[7], feats[13]) and np.array_equal(feats[8], feats[14])
    own = [int(feats[w, j]) for w in (7, 8) for j in (0, 5, 9)]
    assert len(set(own)) == len(own)
    lengths = [m - 2, m - 1, m, m - 2, m - 1, m]
    lists = [(k, some_locations(rng, SMALL_WINDOWS, n, ORDERS[i % 3]), chunks_of(rng, n)) for i, (k, n) in enumerate(zip(own, lengths))]
    lists.append((5, some_locations(rng, SMALL_WINDOWS, 3, "desc"), [3]))
    return Case("existing", SMALL_WINDOWS, batches_of(rng, lists, 2), max_locs=m, real=g, classes={"m-2": own[0::3], "m-1": own[1::3], "m": own[2::3]})


ANC = [0, 0, 1, 1, 2, 3, 4, 5, 6, 7, 8, 9]       # ancestor of the twelve targets of the ambiguity cases; 0 = none
AMBIG_WINDOWS = [50] * len(ANC)
AMBIG_CAP = 8


def _on_targets(rng, tgts):
    return np.array([[int(rng.integers(0, 50)), t] for t in tgts], dtype=np.uint32)


def ambig_lists(rng, max_ambig, used, per=3):
    """item 9 for one max_ambig: -> (lists, classes, stays) with stays[class] = whether the class survives a call with max_ambig"""
    lim = max(max_ambig, 1)
    taxa = [2, 4, 5, 6, 7, 8, 9, 10]              # targets of the different ancestors 1, 2, 3, ...
    fill = lambda n, pool: [pool[i % len(pool)] for i in range(n)]
    shapes = {
        "exact": (taxa[:lim], True),
        "plus1": (taxa[:lim + 1], False),
        "aba": ([2, 4, 3], lim >= 2),                                       # ancestors 1, 2, 1
        "repeat": ([7] * 20, True),
        "anc0": ([0, 1, 0, 1], True),                                       # two targets without a taxon: one taxon
        "anc0plus": ([0] + taxa[:lim], False),
        "single": ([11], True),
        "behind": (fill(AMBIG_CAP, taxa[:lim]) + [taxa[lim]], True),       # the taxon too many is location cap + 1: cut away
        "at_cap": (fill(AMBIG_CAP - 1, taxa[:lim]) + [taxa[lim]], False),  # ... is location cap exactly: counted
    }
    lists, classes, stays = [], {}, {}
    for cname, (tgts, stay) in shapes.items():
        classes[cname] = spread_keys(rng, per, used)
        stays[cname] = stay
        for key in classes[cname]:
            locs = _on_targets(rng, tgts)
            lists.append((key, locs, chunks_of(rng, len(locs))))
    return lists, classes, stays


def ambig_case(max_ambigs, nkeys, seed=9):
    """the classes of every max_ambig in max_ambigs (class names carry it), filled up with singletons to nkeys keys"""
    rng = np.random.default_rng(seed * 1000 + nkeys + sum(max_ambigs))
    used, lists, classes, stays = set(), [], {}, {}
    for a in max_ambigs:
        l, c, s = ambig_lists(rng, a, used)
        lists += l
        classes.update({f"{n}@{a}": v for n, v in c.items()})
        stays.update({f"{n}@{a}": v for n, v in s.items()})
    fillers = spread_keys(rng, nkeys - len(lists), used)
    lists += [(k, _on_targets(rng, [int(rng.integers(0, len(ANC)))]), [1]) for k in fillers]
    c = Case(f"ambig{'_'.join(map(str, max_ambigs))}_{nkeys}", AMBIG_WINDOWS, batches_of(rng, lists, 3), max_locs=AMBIG_CAP, classes=classes, anc=ANC)
    c.stays = stays
    return c


def ambig_all_go_case():
    """every list touches two taxa: a call with max_ambig = 1 leaves no feature"""
    rng = np.random.default_rng(91)
    lists = [(k, _on_targets(rng, [2, 4] + [2] * (i % 3)), [2] + [1] * (i % 3)) for i, k in enumerate(spread_keys(rng, 40, set()))]
    return Case("ambig_all_go", AMBIG_WINDOWS, batches_of(rng, lists, 2), max_locs=AMBIG_CAP, anc=ANC)


def singleton_case(nkeys, name):
    """item 10: nkeys different keys (none 0xFFFFFFFF) with one location each, in no order -- generated and compared vectorised"""
    i = np.arange(nkeys, dtype=np.uint64)
    keys = ((i * np.uint64(2654435761) + np.uint64(12345)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)      # odd multiplier: a bijection of 2^32
    keys[keys == NO_KEY] = np.uint32(((nkeys * 2654435761 + 12345) & 0xFFFFFFFF))
    windows = np.array([1 << 20, 3, 1 << 16], dtype=np.uint64)
    tgt = (i % np.uint64(3)).astype(np.uint32)
    win = ((i * np.uint64(7919)) % windows[tgt]).astype(np.uint32)
    return Case(name, windows, [(keys, np.ones(nkeys, np.uint8), np.stack([win, tgt], axis=1))])


def queries_for(rng, table, extra=()):
    """present keys, absent ones, duplicates, the key that is never stored, in no order"""
    present = rng.choice(table.keys, size=min(len(table.keys), 300)) if len(table.keys) else np.zeros(0, np.uint32)
    absent = rng.integers(0, 1 << 32, size=50, dtype=np.uint64).astype(np.uint32)
    q = np.concatenate([present, absent, present[:20], np.asarray(list(extra) + [NO_KEY, 0, 1], dtype=np.uint32)]).astype(np.uint32)
    return rng.permutation(q)


# ---- the calls ----------------------------------------------------------------------------------------------------------------------
_bound = []


def L():
    """the library with every prototype these tests use beyond api.Builder's own, set in one place"""
    from metacache_amd import api
    lib = api.lib()
    if not _bound:
        lib.mc_build_add_existing_target.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.c_char_p, C.c_uint64, C.c_uint64]
        lib.mc_build_add_locations.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]
        lib.mc_build_reserve.argtypes = [C.c_void_p, C.c_uint64]
        lib.mc_build_finish.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        lib.mc_build_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        lib.mc_build_remove_ambiguous.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
        lib.mc_build_write.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64]
        lib.mc_build_write_shards.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.c_char_p, C.c_void_p, C.c_uint64]
        lib.mc_build_last_error.restype = C.c_char_p
        lib.mc_build_last_error.argtypes = [C.c_void_p]
        _bound.append(True)
    return lib


def pack(vals, target_bytes):
    """{win, tgt}[n] -> the file's packed values: {u32 window, u16 | u32 target}"""
    vals = np.asarray(vals, dtype=np.uint32).reshape(-1, 2)
    out = np.zeros(len(vals), dtype=np.dtype([("win", "<u4"), ("tgt", "<u2" if target_bytes == 2 else "<u4")]))
    assert out.dtype.itemsize == 4 + target_bytes
    out["win"], out["tgt"] = vals[:, 0], vals[:, 1]
    return out


def add_locations(b, keys, sizes, vals, target_bytes):
    """one batch through mc_build_add_locations -> its return code"""
    keys = np.ascontiguousarray(keys, dtype=np.uint32); sizes = np.ascontiguousarray(sizes, dtype=np.uint8)
    raw = pack(vals, target_bytes if target_bytes in (2, 4) else 4)         # (a width the call must refuse: it reads nothing)
    assert len(keys) == len(sizes) and int(sizes.astype(np.int64).sum()) == len(raw)
    dummy = np.zeros(1, dtype=np.uint64)                                    # (an empty batch still hands over three addresses)
    ptr = lambda a: a.ctypes.data if len(a) else dummy.ctypes.data
    return L().mc_build_add_locations(b.h, ptr(keys), ptr(sizes), ptr(raw), len(keys), target_bytes)


def add_existing_target(b, t, windows):
    return L().mc_build_add_existing_target(b.h, f"EXIST_{t:05d}.1".encode(), 0, f"old{t}.fa".encode(), 0, int(windows))


def make_builder(case, shard=0, shards=1):
    """a builder with the case's configuration and existing targets"""
    from metacache_amd import api
    L()
    b = api.Builder(target_id_bytes=case.tb, max_locations_per_feature=case.max_locs, remove_overpopulated=case.rm_over,
                    key_shard_index=shard, key_shard_count=shards, **SMALL_SLOTS)
    for t, w in enumerate(case.windows.tolist()):
        assert add_existing_target(b, t, w) == 0
    return b


def add_batches(b, case):
    """the case's batches in order, then its real targets"""
    for keys, sizes, vals in case.batches:
        rc = add_locations(b, keys, sizes, vals, case.pack)
        assert rc == 0, (rc, L().mc_build_last_error(b.h))
    for i, g in enumerate(case.real):
        b.add_target(g, f"REAL_{i:05d}.1", parent_taxid=0, filename=f"new{i}.fa")


def finish(b):
    b.finish(load=False)
    return b.counts()


def remove_ambiguous(b, anc, max_ambig):
    return b.remove_ambiguous(np.asarray(anc, dtype=np.uint32), max_ambig)


TAXA = [(1, 1, 20, "root")]


def write(builders, name):
    from metacache_amd import api
    if len(builders) == 1:
        builders[0].write(name, TAXA)
    else:
        api.Builder.write_shards(builders, name, TAXA)


def load(builders):
    """the table straight from the builders: mc_build_finish(load) for one, mc_build_finish_shards for a set"""
    from metacache_amd import api
    return builders[0].finish(load=True) if len(builders) == 1 else api.Builder.finish_shards(builders)


def open_file(name):
    from metacache_amd import api
    return api.Database.open(name, **SMALL_SLOTS)


# ---- comparisons --------------------------------------------------------------------------------------------------------------------
def check_file(name, model, case):
    """(b) the written files through the oracle's reader: exactly the model's keys (none missing, none too many, none twice), every
    list in order, the totals of the header and the packing"""
    import cpuref
    odb = cpuref.oracle().open(name)
    try:
        keys, sizes, offs, vals = odb.part_arrays(0)
        assert len(keys) == len(model.keys)
        order = np.argsort(keys, kind="stable")
        assert np.array_equal(keys[order], model.keys)                      # (the model's keys ascend and are distinct)
        assert np.array_equal(sizes[order], model.sizes)
        n = model.sizes.astype(np.int64)
        flat = np.repeat(offs[order].astype(np.int64), n) + (np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n))
        assert np.array_equal(vals[flat], vals64(model))
        assert odb.n_locations == len(model.vals) and odb.n_targets == case.n_targets
        assert odb.ref.lib.mco_db_target_id_bytes(odb.h) == case.tb and odb.max_locs == case.cap
    finally:
        odb.close()


def check_sampled(db, model, sample):
    """(c) for the large tables: histogram and enumeration whole, lookups of `sample` (keys, present or not)"""
    keys, sizes = model.features()
    hist, dead = db.table_histogram()
    assert np.array_equal(hist, np.bincount(sizes, minlength=256)) and dead == 0
    gk, gs = db.table_features()
    assert np.array_equal(gk, keys) and np.array_equal(gs, sizes)
    off, locs = db.table_lookup(sample)
    eoff, elocs = model.lookup(sample)
    assert np.array_equal(off, eoff) and np.array_equal(np.stack([locs["win"], locs["tgt"]], axis=1), elocs)


def check_tables(builders, name, held_model, file_model, case, queries):
    """(c) the table loaded from the builders (overpopulated features held but dead) and the table opened from the written file"""
    db = load(builders)
    try:
        check_table(db, held_model, queries, rm_over=case.cap - 1 if case.rule_on else 0)
        assert db.n_locations == len(file_model.vals) and db.n_targets == case.n_targets
    finally:
        db.close()
    db = open_file(name)
    try:
        check_table(db, file_model, queries)
        assert db.n_locations == len(file_model.vals) and db.n_targets == case.n_targets
    finally:
        db.close()


def run_case(case, tmp_path, shards=1, ambig=()):
    """the case through `shards` builders: (a) counts after finish and after every call of `ambig` = [max_ambig, ...], (b) the files,
    (c) both tables.  -> (held model, file model)"""
    rng = np.random.default_rng(7)
    bs = [make_builder(case, i, shards) for i in range(shards)]
    try:
        models = []
        for i, b in enumerate(bs):
            add_batches(b, case)
            m = held(case, i, shards)
            # mc_build_counts reports what the builder HOLDS: with remove_overpopulated the lists that reached the cap are still there
            # (finish_sorted only cuts them; mc_build_write_add and the table's load filter drop them), so the counts include them
            assert finish(b) == (len(m.keys), len(m.vals)), (case.name, i)
            for a in ambig:
                after = without_ambiguous(m, case.anc, a)
                assert remove_ambiguous(b, case.anc, a) == len(m.keys) - len(after.keys), (case.name, i, a)
                assert b.counts() == (len(after.keys), len(after.vals)), (case.name, i, a)
                m = after
            models.append(m)
        all_held = whole(models)
        in_file = written(all_held, case)
        name = str(tmp_path / case.name)
        write(bs, name)
        check_file(name, in_file, case)
        check_tables(bs, name, all_held, in_file, case, queries_for(rng, all_held, [k for v in case.classes.values() for k in v]))
        return all_held, in_file
    finally:
        for b in bs:
            b.free()
