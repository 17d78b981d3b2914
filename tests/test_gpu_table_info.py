"""GPU: what a loaded table holds -- mc_table_histogram, mc_table_features, mc_table_lookup -- against a numpy model of the arrays the
table was loaded from, in every layout of the store (8-byte, compact, compact with lists on 128-byte lines, 16-bit target ids), against
the reference's recorded feature map for the database files, and for the builder's tables against the file the builder writes."""
import ctypes as C
import os

import numpy as np
import pytest

import table_info_ref as ref
from metacache_amd import api, synth
from table_model import Table, as_pairs, check_table      # noqa: F401 (the model of a table's arrays, shared with the builder's tests)

pytestmark = pytest.mark.gpu

MC_ERR_NOMEM, MC_ERR_UNSUPPORTED, MC_ERR_STATE = -3, -5, -6
LAYOUTS = ["wide", "compact", "aligned", "u16"]
MAX_TGT, MAX_WIN = 40, 5000               # the location range of the tables made here: targets 0 .. 40 with windows 0 .. 5000 each


def mix32(x):
    x = np.asarray(x, dtype=np.uint64)
    x = x ^ (x >> np.uint64(16)); x = (x * np.uint64(0x85ebca6b)) & np.uint64(0xFFFFFFFF)
    x = x ^ (x >> np.uint64(13)); x = (x * np.uint64(0xc2b2ae35)) & np.uint64(0xFFFFFFFF)
    return x ^ (x >> np.uint64(16))


def home_bucket(keys, nbuckets):
    return (mix32(keys) * np.uint64(nbuckets)) >> np.uint64(32)


def load(table, layout, **cfg_kw):
    """the table through mc_load_begin / mc_load_batch / mc_load_end in one of the four layouts -> api.Database"""
    L = api.lib()
    tb = 2 if layout == "u16" else 4
    cfg = api.default_config(target_id_bytes=tb, num_slots=1, slot_max_queries=64, slot_max_chars=1 << 16, **cfg_kw)   # (no queries here: small slots)
    h = C.c_void_p()
    assert L.mc_create(C.byref(cfg), C.byref(h)) == 0, L.mc_last_error(None)
    db = api.Database.from_handle(h.value, cfg)
    try:
        if layout != "wide":
            assert L.mc_load_location_range(db.h, MAX_TGT, MAX_WIN) == 0
        if layout == "aligned":
            db.set_tuning("list_align", 1)
        n, nv = len(table.keys), len(table.vals)
        db._check(L.mc_load_begin(db.h, 0, n, nv))
        if layout == "aligned":
            # lists on 128-byte lines need the padded size of the store before the first batch: the file loaders and the builder announce
            # it through the library's internal announce_store (context.h), which has no C name -- taken by its C++ name here, and the
            # layout is asserted below, so a table that did not get the alignment fails this test instead of passing for the plain one
            announce = getattr(L, "_ZN5mcamd14announce_storeEP6mc_ctxm")
            announce.argtypes = [C.c_void_p, C.c_uint64]
            announce.restype = None
            s = table.sizes.astype(np.int64)
            announce(db.h, int(np.where(s > 1, (s + 31) // 32 * 32, 0).sum()) + 64)
        if tb == 4:
            packed = table.vals
        else:
            packed = np.zeros(nv, dtype=np.dtype([("win", "<u4"), ("tgt", "<u2")]))
            assert packed.dtype.itemsize == 6
            packed["win"], packed["tgt"] = table.vals[:, 0], table.vals[:, 1]
        half = n // 2                                                       # two batches: a list store that is appended to
        v0 = int(table.first[half]) if half < n else nv
        raw = packed.view(np.uint8).reshape(-1)
        db._check(L.mc_load_batch(db.h, 0, table.keys.ctypes.data, table.sizes.ctypes.data, raw.ctypes.data, half))
        if n > half:
            db._check(L.mc_load_batch(db.h, 0, table.keys[half:].ctypes.data, table.sizes[half:].ctypes.data, raw[v0 * (4 + tb):].ctypes.data, n - half))
        db._check(L.mc_load_end(db.h, 0))
        lay = db.table_layout()
        assert lay["location_bytes"] == (8 if layout == "wide" else 4), lay
        assert lay["list_align"] == (32 if layout == "aligned" else 1), lay
        return db
    except Exception:
        db.close()
        raise


def edge_table(rng, nbuckets=None):
    """the sizes at the borders (inline payload, 32 entries = one line of the aligned store, the u8 ceiling), the smallest and largest
    features, locations at (0, 0) and across a target boundary, and -- where nbuckets is known -- twelve keys whose home bucket is the
    table's LAST one: their probe sequence goes to the sibling bucket, then on linearly, which wraps to bucket 0"""
    sizes = [1, 2, 31, 32, 33, 64, 65, 254, 255, 1, 2, 3, 2]
    keys = [0, 1, 0xFFFFFFFE, 77, 1 << 31, 123456789, 0xFFFF0000, 65536, 42, 1000, 1001, 1002, 1003]
    lists = []
    for i, s in enumerate(sizes):
        win = rng.integers(0, MAX_WIN + 1, size=s)
        tgt = rng.integers(0, MAX_TGT + 1, size=s)
        lists.append(np.stack([win, tgt], axis=1))
    lists[9] = np.array([[0, 0]])                                          # a single location at target 0, window 0: an inline payload of 0
    lists[10] = np.array([[0, 0], [MAX_WIN, MAX_TGT]])                     # the first and the last location there is
    lists[11] = np.array([[MAX_WIN, 6], [0, 7], [1, 7]])                   # the last window of a target and the first of the next
    lists[12] = np.array([[MAX_WIN, 0], [0, 1]])
    crowd = 12
    if nbuckets is not None:
        cand = rng.integers(2000, 1 << 32, size=400_000, dtype=np.uint64).astype(np.uint32)
        cand = np.unique(cand[home_bucket(cand, nbuckets) == nbuckets - 1])
        assert len(cand) >= crowd
        extra = cand[:crowd]
    else:
        extra = np.arange(5000, 5000 + crowd, dtype=np.uint32)
    for k in extra:
        s = int(rng.integers(1, 4))
        keys.append(int(k)); sizes.append(s)
        lists.append(np.stack([rng.integers(0, MAX_WIN + 1, size=s), rng.integers(0, MAX_TGT + 1, size=s)], axis=1))
    return Table(keys, sizes, np.concatenate(lists)), np.asarray(extra, dtype=np.uint32)


@pytest.fixture(scope="module")
def edge():
    """nbuckets from a first load with the same number of keys, then the table whose crowd is aimed at the last bucket"""
    probe, _ = edge_table(np.random.default_rng(1))
    db = load(probe, "wide")
    nbuckets = db.table_layout()["buckets"]
    db.close()
    table, crowd = edge_table(np.random.default_rng(1), nbuckets)
    assert len(table.keys) == len(probe.keys) and len(crowd) >= 11 and np.all(home_bucket(crowd, nbuckets) == nbuckets - 1)
    return table, crowd, nbuckets


@pytest.fixture(scope="module")
def big():
    """70 000 random keys, sizes 80 % 1, 15 % 2-3, 5 % 4-255: more than 256 blocks of slots, several tiles of the count / scan / write
    sequences, chunks of the gather -- lists in no particular order of their locations"""
    rng = np.random.default_rng(7)
    n = 70_000
    keys = np.unique(rng.integers(0, 1 << 32, size=n + 2000, dtype=np.uint64).astype(np.uint32))
    keys = rng.permutation(keys)[:n]
    u = rng.random(n)
    sizes = np.where(u < 0.8, 1, np.where(u < 0.95, rng.integers(2, 4, size=n), rng.integers(4, 256, size=n))).astype(np.uint8)
    nv = int(sizes.astype(np.int64).sum())
    vals = np.stack([rng.integers(0, MAX_WIN + 1, size=nv), rng.integers(0, MAX_TGT + 1, size=nv)], axis=1)
    return Table(keys, sizes, vals)


def mixed_queries(rng, table, n):
    """present keys, absent ones between them, duplicates, in no order"""
    present = rng.choice(table.keys, size=n)
    absent = rng.integers(0, 1 << 32, size=n // 2, dtype=np.uint64).astype(np.uint32)
    q = np.concatenate([present, absent, present[: n // 4]])
    return rng.permutation(q)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_edge_table(edge, layout):
    table, crowd, nbuckets = edge
    db = load(table, layout)
    try:
        assert db.table_layout()["buckets"] == nbuckets                     # (the crowd sits where it was aimed)
        q = np.concatenate([[5], table.keys[:3], [2, 0xFFFFFFFD, 0xFFFFFFFF], crowd[::-1], table.keys[3:13], crowd[:2], [0, 0]]).astype(np.uint32)
        check_table(db, table, q)
        off, locs = db.table_lookup(crowd)
        assert np.array_equal(np.diff(off.astype(np.int64)), table.sizes[-len(crowd):])   # every key of the long probe sequence is found
        off, locs = db.table_lookup(np.zeros(0, dtype=np.uint32))           # n == 0
        assert off.tolist() == [0] and len(locs) == 0
        off, locs = db.table_lookup(np.array([2, 3, 4], dtype=np.uint32))   # nothing found: no gather
        assert off.tolist() == [0, 0, 0, 0] and len(locs) == 0
    finally:
        db.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_big_table(big, layout):
    db = load(big, layout)
    try:
        check_table(db, big, mixed_queries(np.random.default_rng(11), big, 5000))
    finally:
        db.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_capacity_is_respected_to_the_entry(edge, layout):
    """capacity one short of the total: MC_ERR_NOMEM, offsets complete, no entry of locs written; the exact capacity: nothing beyond"""
    table, crowd, _ = edge
    L = api.lib()
    db = load(table, layout)
    try:
        q = np.concatenate([table.keys, crowd[:3]]).astype(np.uint32)
        eoff, elocs = table.lookup(q)
        total = int(eoff[-1])
        guard, mark = 8, np.uint64(0xABABABABABABABAB)
        for cap in (total - 1, total):
            buf = np.full(total + 2 * guard, mark, dtype=np.uint64)
            off = np.full(len(q) + 1, np.uint64(0xCDCDCDCDCDCDCDCD), dtype=np.uint64)
            rc = L.mc_table_lookup(db.h, q.ctypes.data, len(q), off.ctypes.data, buf[guard:].ctypes.data, cap, 0)
            assert np.array_equal(off, eoff)
            if cap < total:
                assert rc == MC_ERR_NOMEM and str(total) in L.mc_last_error(db.h).decode()
                assert np.all(buf == mark)
            else:
                assert rc == 0
                assert np.all(buf[:guard] == mark) and np.all(buf[guard + total:] == mark)
                got = buf[guard:guard + total]
                assert np.array_equal(np.stack([got & np.uint64(0xFFFFFFFF), got >> np.uint64(32)], axis=1), elocs)
        num = C.c_uint64()
        k2 = np.full(4, 0xABABABAB, dtype=np.uint32); s2 = np.full(4, 0xABABABAB, dtype=np.uint32)
        assert L.mc_table_features(db.h, k2.ctypes.data, s2.ctypes.data, 2, C.byref(num), 0) == 0      # the first `capacity`, num = all
        keys, sizes = table.features()
        assert num.value == len(keys) and np.array_equal(k2[:2], keys[:2]) and np.array_equal(s2[:2], sizes[:2]) and np.all(k2[2:] == 0xABABABAB) and np.all(s2[2:] == 0xABABABAB)
    finally:
        db.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_load_time_rules(big, edge, layout):
    """max_locations_per_feature = 2: the first two of each list; remove_overpopulated = 3: those features are not enumerated, look up
    empty, and `dead` counts them"""
    rng = np.random.default_rng(13)
    for table in (edge[0], big):
        q = mixed_queries(rng, table, 2000)
        db = load(table, layout, max_locations_per_feature=2)
        try:
            check_table(db, table, q, max_locs=2)
        finally:
            db.close()
        db = load(table, layout, remove_overpopulated=3)
        try:
            check_table(db, table, q, rm_over=3)
            assert db.table_histogram()[1] == int((table.sizes > 3).sum()) > 0
        finally:
            db.close()


def test_what_the_calls_do_not_support(edge, golden):
    L = api.lib()
    hist = np.zeros(256, dtype=np.uint64)
    off = np.zeros(2, dtype=np.uint64)
    key = np.zeros(1, dtype=np.uint32)
    num = C.c_uint64()

    def refused(db, code, word):
        for rc in (L.mc_table_histogram(db.h, hist.ctypes.data, None), L.mc_table_features(db.h, None, None, 0, C.byref(num), 0),
                   L.mc_table_lookup(db.h, key.ctypes.data, 1, off.ctypes.data, None, 0, 0)):
            assert rc == code and word in L.mc_last_error(db.h).decode(), (rc, L.mc_last_error(db.h))

    db = api.Database.open(golden.db_path("toy32p2"))                       # two parts in one context
    try:
        refused(db, MC_ERR_UNSUPPORTED, "parts")
    finally:
        db.close()
    db = load(edge[0], "compact", key_shard_index=0, key_shard_count=2)
    try:
        refused(db, MC_ERR_UNSUPPORTED, "key shard")
    finally:
        db.close()
    db = api.Database.open(golden.db_path("toy32"), target_shard_index=0, target_shard_count=2)
    try:
        refused(db, MC_ERR_UNSUPPORTED, "target-range shard")
    finally:
        db.close()
    cfg = api.default_config(target_id_bytes=4)                             # a table that is not finished
    h = C.c_void_p()
    assert L.mc_create(C.byref(cfg), C.byref(h)) == 0
    db = api.Database.from_handle(h.value, cfg)
    try:
        refused(db, MC_ERR_STATE, "not finished")
        db._check(L.mc_load_begin(db.h, 0, 4, 4))
        refused(db, MC_ERR_STATE, "not finished")
    finally:
        db.close()


def check_against_recorded(db, counts, lists):
    """a part's table against the reference's recorded lines: features, sizes, lists and the histogram"""
    keys, sizes = db.table_features()
    want = sorted(counts)
    assert keys.tolist() == want and sizes.tolist() == [counts[k] for k in want]
    hist, dead = db.table_histogram()
    assert hist.tolist() == ref.histogram(counts.values()) and dead == 0
    if lists is not None:
        off, locs = db.table_lookup(keys)
        got = {int(k): list(zip(locs["tgt"][int(a):int(b)].tolist(), locs["win"][int(a):int(b)].tolist())) for k, a, b in zip(keys, off[:-1], off[1:])}
        assert got == lists
    return hist, dead


@pytest.mark.parametrize("pipeline", ["1", "0"])
@pytest.mark.parametrize("name", ["toy32", "toy16"])
def test_database_files(golden, monkeypatch, name, pipeline):
    """the table a file loader leaves (the pipelined one and MC_LOAD_PIPELINE=0) holds what the reference prints for the file"""
    monkeypatch.setenv("MC_LOAD_PIPELINE", pipeline)
    db = api.Database.open(golden.db_path(name))
    try:
        hist, dead = check_against_recorded(db, ref.counts_of(name)[0], ref.lists_of(name)[0])
        got = ref.size_lines(api.table_statistics(hist, dead))
        blk = ref.size_blocks(name)[0]
        assert {k: blk[k] for k in got} == got
    finally:
        db.close()


@pytest.mark.parametrize("name,part", [("toy32p2", 0), ("toy32p2", 1), ("toy32p4", 3)])
def test_single_parts_of_a_database(golden, name, part):
    db = api.Database.open(golden.db_path(name), single_part=part)
    try:
        check_against_recorded(db, ref.counts_of(name)[part], ref.lists_of(name)[part] if name in ref.MAP_DBS else None)
    finally:
        db.close()


def test_the_builders_table_equals_its_file(tmp_path):
    rng = np.random.default_rng(3)
    repeat = synth.random_genome(rng, 600)
    bld = api.Builder(target_id_bytes=4, max_candidates=2)
    for i in range(12):
        g = synth.random_genome(rng, 6000 + 37 * i)
        g[1120:1720] = repeat                                               # lists of 12 and more beside the singletons
        bld.add_target(g, f"SYN_{i:05d}.1", parent_taxid=1000, filename=f"f{i}.fa")
    built = bld.finish(load=True)
    try:
        name = str(tmp_path / "built")
        bld.write(name, [(1, 1, 20, "root"), (1000, 1, 4, "species")])
        bld.free()
        k1, s1 = built.table_features()
        o1, l1 = built.table_lookup(k1)
        h1, d1 = built.table_histogram()
    finally:
        built.close()
    db = api.Database.open(name)
    try:
        k2, s2 = db.table_features()
        o2, l2 = db.table_lookup(k2)
        h2, d2 = db.table_histogram()
    finally:
        db.close()
    assert len(k1) > 500 and s1.max() >= 12
    assert np.array_equal(k1, k2) and np.array_equal(s1, s2) and np.array_equal(o1, o2) and np.array_equal(l1, l2) and np.array_equal(h1, h2)
    assert d2 == 0
