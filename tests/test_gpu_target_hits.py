"""GPU: mc_target_hits_reserve / _add / _collect against the numpy model of target_hits_ref.py, exact (byte for byte).

Contexts without a database (mc_create + mc_set_lineages), lineages with holes; the end to end cases run on the golden toy database
with the candidates of real reads.  T is the block sort's tile, read from the library."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import target_hits_ref as ref
from metacache_amd import api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUM_RANKS = 21
MC_OK, MC_ERR_INVALID, MC_ERR_NOMEM, MC_ERR_STATE = 0, -1, -3, -6
BLOCK, MAX_BLOCKS = 256, 2048                                       # the append kernel's block and its capped grid
BIG = 2 ** 32


def make_lineages(rng, nt):
    """[nt, 21] taxon index + 1 with holes: some targets without a sequence-level taxon, some without anything above it, some empty"""
    lin = np.zeros((nt, NUM_RANKS), dtype=np.uint32)
    lin[:, 0] = np.arange(1, nt + 1)
    for r in range(1, NUM_RANKS):
        lin[:, r] = nt + 1 + 40 * r + (np.arange(nt) * max(1, 40 - 2 * r)) // nt
    lin[:, 1:][rng.random((nt, NUM_RANKS - 1)) < 0.5] = 0
    lin[rng.random(nt) < 0.06, 0] = 0
    lin[rng.random(nt) < 0.04] = 0
    return lin


class Table:
    """a context with lineages, and the device side of the calls"""

    def __init__(self, lin):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        cfg = api.default_config()
        h = C.c_void_p()
        assert api.lib().mc_create(C.byref(cfg), C.byref(h)) == 0, api.lib().mc_last_error(None)
        self.db = api.Database.from_handle(h.value, cfg)
        self.set(lin)

    def set(self, lin):
        self.lin = lin
        self.db.set_lineages(lin)

    def to_device(self, cands, ids=None):
        n, stride = cands.shape
        flat = np.ascontiguousarray(cands).view(np.uint32).reshape(n, stride * 4).view(np.int32)
        d = self.torch.from_numpy(flat.copy()).to(self.dev) if n else self.torch.zeros((1, stride * 4), dtype=self.torch.int32, device=self.dev)
        q = None if ids is None else self.torch.from_numpy(np.ascontiguousarray(ids, dtype=np.uint64).view(np.int64).copy()).to(self.dev)
        return d, q

    def add(self, cands, ids=None, first=0, hitmin=0, lowest=0, stream=0):
        """appends on the device; the tensors are returned so that they outlive the asynchronous call"""
        d, q = self.to_device(cands, ids)
        self.torch.cuda.synchronize()
        self.db.target_hits_add_device(d.data_ptr(), cands.shape[0], cands.shape[1], query_ids_ptr=q.data_ptr() if q is not None and len(cands) else 0,
                                       first_query_id=first, hitmin=hitmin, lowest=lowest, stream=stream)
        return d, q

    def empty(self, capacity):
        """an empty log of `capacity` records"""
        self.db.target_hits_stats(reset=True)
        self.db.target_hits_reserve(0)
        if capacity:
            self.db.target_hits_reserve(capacity)

    def want(self, cands, ids=None, first=0, hitmin=0, lowest=0):
        return ref.records_of(self.lin, cands, hitmin, lowest, ids, first)

    def check(self, rec, calls=1):
        """collect == the model on the records `rec` (any order)"""
        off, got, st = self.db.target_hits_collect()
        woff, wrec, whit = ref.collect(rec, len(self.lin))
        assert got.dtype == wrec.dtype and len(got) == len(wrec)
        if got.tobytes() != wrec.tobytes():
            bad = np.flatnonzero(got != wrec)
            raise AssertionError((len(bad), bad[:3], got[bad[:3]], wrec[bad[:3]]))
        assert off.tobytes() == woff.tobytes()
        assert st == dict(stored=len(wrec), dropped=0, calls=calls, targets_hit=whit), st
        return off, got

    def one_call(self, cands, ids=None, first=0, hitmin=0, lowest=0, slack=0):
        rec = self.want(cands, ids, first, hitmin, lowest)
        self.empty(len(rec) + slack if len(rec) + slack else 1)
        keep = self.add(cands, ids, first, hitmin, lowest)
        out = self.check(rec, calls=1 if len(cands) else 0)
        del keep
        return rec, out

    def close(self):
        self.db.close()


@pytest.fixture(scope="module")
def table():
    rng = np.random.default_rng(2025)
    t = Table(make_lineages(rng, 300))
    yield t
    t.close()


@pytest.fixture(scope="module")
def tile():
    return api.target_hits_tile()


def random_rows(rng, n, stride, nt):
    """targets over the table and a few beyond it, rows that end early, window numbers over the whole 32-bit range"""
    c = np.zeros((n, stride), dtype=api.cand_dtype)
    tgt = rng.integers(0, nt, size=(n, stride))
    tgt = np.where(rng.random((n, stride)) < 0.02, rng.choice(np.array([nt, nt + 1, 2 ** 31, 2 ** 32 - 1]), size=(n, stride)), tgt)
    beg = np.where(rng.random((n, stride)) < 0.5, rng.integers(0, 50, size=(n, stride)), rng.integers(0, 2 ** 32, size=(n, stride)))
    end = np.minimum(beg + rng.integers(0, 4, size=(n, stride)), 2 ** 32 - 1)
    hits = rng.integers(1, 40, size=(n, stride))
    hits[rng.random((n, stride)) < 0.1] = 0                                                  # the row ends here, whatever follows
    c["tgt"] = tgt.astype(np.uint32); c["hits"] = hits.astype(np.uint32); c["beg"] = beg.astype(np.uint32); c["end"] = end.astype(np.uint32)
    return c


def rows_of(entries, stride):
    c = np.zeros((len(entries), stride), dtype=api.cand_dtype)
    for i, e in enumerate(entries):
        for j, x in enumerate(e if isinstance(e, list) else [e]):
            c[i, j] = x
    return c


def flat_rows(tgt, beg, end, hits):
    """one qualifying entry per row (stride 1): as many records as rows"""
    c = np.zeros((len(tgt), 1), dtype=api.cand_dtype)
    c["tgt"][:, 0] = tgt; c["beg"][:, 0] = beg; c["end"][:, 0] = end; c["hits"][:, 0] = hits
    return c


def good_targets(lin, lowest=0):
    return np.flatnonzero(ref.tax_all(lin, np.arange(len(lin)), lowest) != 0)


# ---- append ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, BLOCK * MAX_BLOCKS + 1])
def test_append_row_counts_strides_ranks_and_ids(table, n):
    rng = np.random.default_rng(n + 1)
    # a target without a taxon on ranks 0 and 1 (a hole) and with one above them: it qualifies with lowest_rank 1, not with 0
    hole = int(np.flatnonzero((table.lin[:, 0] == 0) & (table.lin[:, 1] == 0) & (table.lin[:, 2:].max(axis=1) > 0))[0])
    assert ref.tax(table.lin, hole, 1) != 0 and ref.tax(table.lin, hole, 0) == 0
    combos = [(s, lo) for s in (1, 2, 4) for lo in (0, 1)] if n <= 257 else [(1, 0), (2, 1), (4, 0)]
    for k, (stride, lowest) in enumerate(combos):
        cands = random_rows(rng, n, stride, len(table.lin))
        if n:
            cands[0, 0] = (hole, 1000, 5, 6)                                      # (hits 1000: no other entry has them)
        ids = rng.integers(0, 2 ** 63, size=n).astype(np.uint64) * np.uint64(2) + np.uint64(1) if k % 2 else None     # beyond 2^32, up to 2^64 - 1
        rec, _ = table.one_call(cands, ids, first=BIG * 5 + 3, hitmin=5, lowest=lowest)
        if n >= 63:
            assert 0 < len(rec) < n * stride
            assert (rec["query"] > BIG).all()
        if n:
            assert (rec["hits"] == 1000).sum() == lowest                                    # qualified by the rank above the hole, and only by it


def test_append_hand_written_rows(table):
    g = good_targets(table.lin)
    bad = int(np.flatnonzero(ref.tax_all(table.lin, np.arange(len(table.lin)), 0) == 0)[0])
    a, b, c = int(g[0]), int(g[1]), int(g[-1])
    nt = len(table.lin)
    cands = rows_of([
        [],                                                               # an empty row
        [(a, 9, 1, 2), (b, 8, 3, 4), (c, 7, 5, 6), (a, 6, 7, 8)],         # a full row
        [(bad, 9, 1, 1), (a, 9, 2, 2)],                                   # a non-qualifying entry in front of a qualifying one: no taxon ...
        [(nt, 9, 1, 1), (b, 9, 3, 3)],                                    # ... a tgt right beyond the table ...
        [(2 ** 32 - 1, 9, 1, 1), (b, 9, 4, 4)],
        [(a, 4, 1, 1), (c, 5, 9, 9)],                                     # ... hits below hits_min = 5, then at it
        [(a, 6, 11, 11)],                                                 # above it
        [(a, 9, 12, 12), (0, 0, 0, 0), (b, 9, 13, 13)],                   # the row ends at hits == 0
    ], 4)
    ids = np.array([7, BIG + 1, 2 ** 64 - 1, 3, BIG * BIG // 2, 5, 6, BIG - 1], dtype=np.uint64)
    rec, (off, got) = table.one_call(cands, ids, hitmin=5)
    assert len(rec) == 4 + 1 + 1 + 1 + 1 + 1 + 1
    assert sorted(int(q) for q in got["query"][got["tgt"] == a]) == sorted([BIG + 1, BIG + 1, 2 ** 64 - 1, 6, BIG - 1])
    rec, _ = table.one_call(cands, None, first=2 ** 64 - 8, hitmin=5)                        # no ids: first_query_id + i, up to 2^64 - 1
    assert int(rec["query"].max()) == 2 ** 64 - 1
    assert len(table.one_call(cands, ids, hitmin=4)[0]) == 11 and len(table.one_call(cands, ids, hitmin=6)[0]) == 9
    assert len(table.one_call(cands, ids, hitmin=10)[0]) == 0


# ---- capacity ------------------------------------------------------------------------------------------------------------------------------
def raw_collect(db, want_records, n_targets, n_records):
    L = api.lib()
    nt, nr = C.c_uint64(), C.c_uint64()
    st = np.zeros(4, dtype=np.uint64)
    off = np.zeros(n_targets + 1, dtype=np.uint64)
    rec = np.zeros(max(n_records, 1), dtype=api.target_hit_dtype)
    rc = L.mc_target_hits_collect(db.h, off.ctypes.data if want_records else None, n_targets, C.byref(nt), rec.ctypes.data if want_records else None,
                                  n_records, C.byref(nr), st.ctypes.data, 0)
    return rc, int(nt.value), int(nr.value), st.tolist()


def test_a_full_log_drops_nothing_and_one_short_drops_one(table):
    rng = np.random.default_rng(11)
    cands = random_rows(rng, 1000, 2, len(table.lin))
    rec = table.want(cands, hitmin=3)
    table.empty(len(rec))
    keep = table.add(cands, hitmin=3)
    table.check(rec)                                                       # exactly full: dropped == 0
    table.empty(len(rec) - 1)
    keep = table.add(cands, hitmin=3)
    st = table.db.target_hits_stats()                                      # the size query answers
    assert (st["records"], st["stored"], st["dropped"], st["calls"], st["targets"]) == (len(rec) - 1, len(rec) - 1, 1, 1, len(table.lin))
    rc, nt, nr, stats = raw_collect(table.db, True, len(table.lin), len(rec))
    assert rc == MC_ERR_STATE and (nt, nr) == (len(table.lin), len(rec) - 1) and stats[1] == 1
    with pytest.raises(api.McError):
        table.db.target_hits_collect()
    assert raw_collect(table.db, False, 0, 0)[0] == MC_OK
    assert api.lib().mc_target_hits_add(table.db.h, cands.ctypes.data, None, 0, 10, 2, 0, 0, api.TARGET_HITS_HOST, None) == MC_ERR_STATE   # host mode does not build on a log with holes
    table.db.target_hits_stats(reset=True)
    assert table.db.target_hits_stats()["dropped"] == 0
    del keep


def test_capacities_smaller_than_the_size_are_invalid(table):
    rng = np.random.default_rng(12)
    cands = random_rows(rng, 100, 2, len(table.lin))
    rec, _ = table.one_call(cands)
    assert len(rec) > 2
    assert raw_collect(table.db, True, len(table.lin) - 1, len(rec))[0] == MC_ERR_INVALID
    assert raw_collect(table.db, True, len(table.lin), len(rec) - 1)[0] == MC_ERR_INVALID
    assert raw_collect(table.db, True, len(table.lin), len(rec))[0] == MC_OK
    assert api.lib().mc_target_hits_reserve(table.db.h, len(rec) - 1) == MC_ERR_INVALID      # what the log holds stays
    table.db.target_hits_reserve(len(rec) + 100)
    table.check(rec)


def test_device_mode_needs_a_reserved_log_and_host_mode_grows_from_nothing(table):
    rng = np.random.default_rng(13)
    cands = random_rows(rng, 3000, 4, len(table.lin))
    table.empty(0)
    d, _ = table.to_device(cands)
    table.torch.cuda.synchronize()
    assert api.lib().mc_target_hits_add(table.db.h, d.data_ptr(), None, 0, 3000, 4, 0, 0, 0, None) == MC_ERR_STATE
    assert table.db.target_hits_stats()["records"] == 0
    ids = rng.integers(0, 2 ** 64, size=3000, dtype=np.uint64)
    table.db.target_hits_add(cands[:1000], ids[:1000], hitmin=2, lowest=1)
    table.db.target_hits_add(cands[1000:], None, first_query_id=BIG * 9, hitmin=2, lowest=1)
    for _ in range(12):                                                    # room is made again and again: doubling, with what the log holds copied over
        table.db.target_hits_add(cands[:2000], ids[:2000], hitmin=2, lowest=1)
    rec = np.concatenate([table.want(cands[:1000], ids[:1000], 0, 2, 1), table.want(cands[1000:], None, BIG * 9, 2, 1)] +
                         [table.want(cands[:2000], ids[:2000], 0, 2, 1)] * 12)
    assert len(rec) > 65536                                                # (the first allocation's size)
    table.check(rec, calls=14)


def test_host_mode_beyond_target_hits_max_mb_adds_nothing(table):
    rng = np.random.default_rng(14)
    cands = random_rows(rng, 20_000, 2, len(table.lin))
    table.empty(0)
    table.db.set_tuning("target_hits_max_mb", 1)                           # 43 690 records
    try:
        table.db.target_hits_add(cands)                                    # room for 40 000 more
        rec = table.want(cands)
        assert 20_000 < len(rec) < 40_000
        rc = api.lib().mc_target_hits_add(table.db.h, cands.ctypes.data, None, 0, 20_000, 2, 0, 0, api.TARGET_HITS_HOST, None)
        assert rc == MC_ERR_NOMEM                                          # len(rec) + 40 000 is more than 1 MiB holds
        table.check(rec)                                                   # the log as it was
        table.db.target_hits_add(cands[:1000])                             # a batch that fits is still taken
        table.check(np.concatenate([rec, table.want(cands[:1000])]), calls=2)
    finally:
        table.db.set_tuning("target_hits_max_mb", 8192)


@pytest.mark.parametrize("with_ids", [True, False])
def test_host_mode_beyond_one_staged_piece_numbers_the_queries_of_the_second_piece(table, with_ids):
    """MC_TARGET_HITS_HOST stages 64 MB pieces: 2^20 rows of stride 4; one row more starts a second piece, which reads query_ids + 2^20
    or counts on from first_query_id + 2^20.  All rows are empty but a handful on both sides of the border (the last row is the second
    piece), so the model only has to look at those; every filled row has a `beg` of its own to find its records by."""
    stride = 4
    piece = (64 << 20) // (stride * 16)
    n = piece + 1
    rng = np.random.default_rng(15)
    g = good_targets(table.lin)
    bad = int(np.flatnonzero(ref.tax_all(table.lin, np.arange(len(table.lin)), 0) == 0)[0])
    filled = [0, 77, piece - 3, piece - 2, piece - 1, n - 1]
    cands = np.zeros((n, stride), dtype=api.cand_dtype)
    for k, r in enumerate(filled):
        beg = 1000 + k
        cands[r] = rows_of([[(int(g[k]), 9, beg, beg + 1), (bad, 9, beg, beg), (int(g[-1 - k]), 8, beg, beg + 2), (int(g[k]), 7, beg, beg + 3)][: 1 + (k + 3) % stride]], stride)[0]
    first = BIG * 3 + 11
    ids = rng.integers(0, 2 ** 64, size=n, dtype=np.uint64) if with_ids else None
    query_of = (lambda r: int(ids[r])) if with_ids else (lambda r: first + r)
    rec = ref.records_of(table.lin, cands[filled], 0, 0, np.array([query_of(r) for r in filled], dtype=np.uint64))
    assert len(filled) < len(rec) < len(filled) * stride
    table.empty(0)                                                         # (the call reserves n * stride records: 100 MB)
    try:
        table.db.target_hits_add(cands, ids, first_query_id=first)
        off, got = table.check(rec)
        for k, r in enumerate(filled):
            mine = got[got["beg"] == 1000 + k]
            assert len(mine) > 0 and (mine["query"] == np.uint64(query_of(r))).all(), (r, mine)
    finally:
        table.empty(0)


# ---- the sort ------------------------------------------------------------------------------------------------------------------------------
def passes_of(n, tile):
    tiles, p = -(-n // tile), 0
    while tiles > 1:
        tiles, p = -(-tiles // 2), p + 1
    return p


COUNTS = {"0": lambda T: 0, "1": lambda T: 1, "T-1": lambda T: T - 1, "T": lambda T: T, "T+1": lambda T: T + 1,
          "2T+1": lambda T: 2 * T + 1,                                  # a short last run
          "3T": lambda T: 3 * T,                                        # a run without a partner
          "5T+7": lambda T: 5 * T + 7}                                  # three passes


@pytest.mark.parametrize("count", list(COUNTS))
def test_sort_record_counts(table, tile, count):
    n = COUNTS[count](tile)
    assert {"T+1": 1, "2T+1": 2, "3T": 2, "5T+7": 3}.get(count, 0) == passes_of(n, tile)     # both parities of the number of passes
    rng = np.random.default_rng(n + 7)
    g = good_targets(table.lin)
    cands = flat_rows(rng.choice(g, size=n), rng.integers(0, 30, size=n), rng.integers(30, 34, size=n), rng.integers(1, 9, size=n))
    ids = rng.integers(0, 2 ** 64, size=n, dtype=np.uint64)
    rec, _ = table.one_call(cands, ids)
    assert len(rec) == n
    # the size query sorts, the full call finds the log sorted; a second collect returns the same
    table.check(rec, calls=1 if n else 0)


@pytest.mark.parametrize("shape", ["one_target", "only_query_differs", "only_hits_differ", "all_equal", "descending"])
def test_sort_data_shapes(table, tile, shape):
    n = 5 * tile + 7
    rng = np.random.default_rng(len(shape))
    g = good_targets(table.lin)
    one = np.full(n, int(g[3]))
    if shape == "one_target":
        cands, ids = flat_rows(one, rng.integers(0, 9, size=n), rng.integers(9, 12, size=n), rng.integers(1, 5, size=n)), rng.integers(0, 2 ** 64, size=n, dtype=np.uint64)
    elif shape == "only_query_differs":
        cands, ids = flat_rows(one, 4, 6, 3), rng.permutation(n).astype(np.uint64) * np.uint64(BIG // 2 + 1)       # distinct, on both sides of 2^32
    elif shape == "only_hits_differ":
        cands, ids = flat_rows(one, 4, 6, rng.permutation(n) + 1), np.full(n, BIG + 5, dtype=np.uint64)
    elif shape == "all_equal":
        cands, ids = flat_rows(one, 4, 6, 3), np.full(n, BIG + 5, dtype=np.uint64)
        cands["tgt"][: n // 3, 0] = int(g[1])                              # (two runs of duplicates, so that the order is visible at all)
    else:
        k = np.arange(n)[::-1]
        cands, ids = flat_rows(g[k * len(g) // n], k, k + 1, 2), (k.astype(np.uint64) << np.uint64(20))
        chk = ref.records_of(table.lin, cands, 0, 0, ids)
        assert ref.sort_records(chk).tobytes() == chk[::-1].tobytes()      # the input is the sorted order backwards
    rec, _ = table.one_call(cands, ids)
    assert len(rec) == n


# ---- bounds ------------------------------------------------------------------------------------------------------------------------------
def test_bounds_with_empty_targets_at_the_ends_and_in_the_middle():
    nt = 700
    lin = np.zeros((nt, NUM_RANKS), dtype=np.uint32)
    lin[:, 0] = np.arange(1, nt + 1)
    t = Table(lin)
    try:
        rng = np.random.default_rng(21)
        allowed = np.concatenate([np.arange(1, 200), np.arange(460, nt - 1)])               # 0 and nt - 1 empty, 200 .. 459 empty (more than a block of lanes)
        n = 8000
        cands = flat_rows(rng.choice(allowed, size=n), rng.integers(0, 9, size=n), 9, 1)
        rec, (off, _) = t.one_call(cands)
        cnt = np.diff(off.astype(np.int64))
        assert cnt[0] == 0 and cnt[-1] == 0 and (cnt[200:460] == 0).all() and cnt.sum() == n and int(off[-1]) == n
        assert (cnt[1:200] > 0).all()
        lin1 = np.zeros((1, NUM_RANKS), dtype=np.uint32)
        lin1[0, 0] = 1
        t.set(lin1)                                                        # a single target
        cands = flat_rows(np.zeros(n, dtype=np.int64), rng.integers(0, 9, size=n), 9, 1)
        cands["tgt"][::7, 0] = 1                                           # beyond the table: not recorded
        rec, (off, _) = t.one_call(cands)
        assert off.tolist() == [0, len(rec)] and len(rec) == n - len(range(0, n, 7))
        t.empty(4)
        assert t.db.target_hits_collect()[0].tolist() == [0, 0]            # an empty log
    finally:
        t.close()


# ---- determinism, reset ---------------------------------------------------------------------------------------------------------------------
def test_call_order_and_streams_do_not_change_the_result(table):
    torch = table.torch
    rng = np.random.default_rng(31)
    n = 60_000
    cands = random_rows(rng, n, 2, len(table.lin))
    ids = rng.integers(0, 2 ** 64, size=n, dtype=np.uint64)
    rec = table.want(cands, ids, hitmin=4)
    results = []
    # one call
    table.empty(len(rec))
    keep = [table.add(cands, ids, hitmin=4)]
    results.append(table.check(rec, calls=1))
    # several calls, the pieces in reversed order
    cuts = [0, 1, 700, 20_000, 20_064, n]
    table.empty(len(rec))
    for lo, hi in reversed(list(zip(cuts[:-1], cuts[1:]))):
        keep.append(table.add(cands[lo:hi], ids[lo:hi], hitmin=4))
    results.append(table.check(rec, calls=len(cuts) - 1))
    # two streams of the caller at the same time
    table.empty(len(rec))
    streams = [torch.cuda.Stream(device=table.dev) for _ in range(2)]
    halves = [table.to_device(cands[: n // 2], ids[: n // 2]), table.to_device(cands[n // 2:], ids[n // 2:])]
    torch.cuda.synchronize()
    for (d, q), s, m in zip(halves, streams, (n // 2, n - n // 2)):
        table.db.target_hits_add_device(d.data_ptr(), m, 2, query_ids_ptr=q.data_ptr(), hitmin=4, stream=s.cuda_stream)
    for s in streams:
        s.synchronize()
    results.append(table.check(rec, calls=2))
    for off, got in results[1:]:
        assert off.tobytes() == results[0][0].tobytes() and got.tobytes() == results[0][1].tobytes()
    del keep, halves


def test_reset_clears_and_new_lineages_drop_the_log():
    rng = np.random.default_rng(41)
    lin = make_lineages(rng, 120)
    t = Table(lin)
    try:
        cands = random_rows(rng, 5000, 2, len(lin))
        rec, _ = t.one_call(cands, slack=10)
        assert len(rec) > 1000
        off, got, st = t.db.target_hits_collect(reset=True)                # read, then cleared
        assert len(got) == len(rec) and st["calls"] == 1
        st = t.db.target_hits_stats()
        assert (st["records"], st["stored"], st["dropped"], st["calls"], st["targets_hit"]) == (0, 0, 0, 0, 0)
        keep = t.add(cands[:100])                                          # the log is still reserved
        t.check(t.want(cands[:100]))
        lin2 = make_lineages(rng, 90)
        t.set(lin2)                                                        # mc_set_lineages drops what was accumulated
        st = t.db.target_hits_stats()
        assert (st["targets"], st["records"], st["calls"]) == (90, 0, 0)
        cands2 = random_rows(rng, 2000, 2, len(lin2))
        keep = t.add(cands2, first=17)
        t.check(t.want(cands2, first=17))
        t.db.timing(True)                                                  # the collect-side kernels are timed under their names
        t.db.timing_reset()
        keep = t.add(cands2[:50])
        t.db.target_hits_collect()
        assert t.db.timing_get("target_hits_sort")[1] == 1 and t.db.timing_get("target_hits_bounds")[1] >= 1
        del keep
    finally:
        t.close()


# ---- end to end on the golden toy database --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def example(tmp_path_factory):
    """examples/target_hits_example.cpp, compiled once into a temporary directory (nothing is written into the source tree)"""
    from metacache_amd import build
    build.build_library()
    exe = str(tmp_path_factory.mktemp("target_hits_example") / "target_hits_example")
    cmd = ["g++", "-std=c++14", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "target_hits_example.cpp"),
           "-L" + os.path.join(ROOT, "metacache_amd", "lib"), "-lmetacache_amd", "-Wl,-rpath," + os.path.join(ROOT, "metacache_amd", "lib"),
           "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def lines_of(off, rec):
    out = []
    for t in range(len(off) - 1):
        lo, hi = int(off[t]), int(off[t + 1])
        if lo < hi:
            out.append(f"{t}\t{hi - lo}\t" + ",".join(f"{int(r['query'])}/{int(r['beg'])}+{int(r['end']) - int(r['beg'])}:{int(r['hits'])}" for r in rec[lo:hi]))
    return out


@pytest.mark.parametrize("hitmin,lowest", [(0, 0), (3, 0), (2, 6)])
def test_toy_database_candidates_equal_the_model(golden, hitmin, lowest):
    single, _, _ = golden.reads()
    reads = single[:600]
    db = api.Database.open(golden.db_path("toy32"), max_candidates=2)
    try:
        cands, _, _ = db.query(reads, lowest=lowest)
        lin = db.lineages()
        db.target_hits_add(cands[:250], first_query_id=1, hitmin=hitmin, lowest=lowest)
        db.target_hits_add(cands[250:], first_query_id=251, hitmin=hitmin, lowest=lowest)
        off, rec, st = db.target_hits_collect(reset=True)
    finally:
        db.close()
    woff, wrec, whit = ref.collect(ref.records_of(lin, cands, hitmin, lowest, first_query_id=1), len(lin))
    assert len(wrec) > 300 and whit >= 2
    assert rec.tobytes() == wrec.tobytes() and off.tobytes() == woff.tobytes()
    assert st == dict(stored=len(wrec), dropped=0, calls=2, targets_hit=whit)


def test_cpp_example_prints_what_the_python_binding_returns(golden, example, tmp_path):
    single, _, _ = golden.reads()
    reads = [r for r in single[:400] if b"\n" not in r and len(r) > 0]
    f = tmp_path / "seqs.txt"
    f.write_bytes(b"\n".join(reads) + b"\n")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    out = subprocess.check_output([example, golden.db_path("toy32"), str(f), "2"], env=env).decode().splitlines()
    db = api.Database.open(golden.db_path("toy32"), max_candidates=2)
    try:
        cands, _, _ = db.query(reads)
        db.target_hits_add(cands, hitmin=2)
        off, rec, _ = db.target_hits_collect(reset=True)
    finally:
        db.close()
    want = lines_of(off, rec)
    assert len(want) >= 2 and out == want
