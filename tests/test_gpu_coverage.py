"""GPU: mc_coverage_add / _counts / _set_keep / _drop against the numpy model of coverage_ref.py, exact.

Tables of a few hundred small targets announced with mc_load_target_windows + mc_set_lineages on a context without a database; the end
to end cases run on the golden toy database with the candidates of real reads."""
import ctypes as C
import os

import numpy as np
import pytest

import classify_ref
import coverage_ref
from metacache_amd import api

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NUM_RANKS = 21
MC_ERR_STATE = -6
BLOCK, MAX_BLOCKS = 256, 2048                                       # the marking kernel's block and its capped grid
EDGE_WINDOWS = [1, 31, 32, 33, 2048, 2049, 2016, 2080]              # words per target: 1, 1, 1, 2, 64, 65, 63, 65


def make_windows(rng, nt):
    w = rng.integers(1, 20_000, size=nt).astype(np.uint32)
    w[: len(EDGE_WINDOWS)] = EDGE_WINDOWS
    w[-len(EDGE_WINDOWS):] = EDGE_WINDOWS[::-1]                      # (the last target has one window)
    return w


def make_lineages(rng, nt):
    """[nt, 21] taxon index + 1 with holes: some targets without a sequence-level taxon, some without anything above it, some empty"""
    lin = np.zeros((nt, NUM_RANKS), dtype=np.uint32)
    lin[:, 0] = np.arange(1, nt + 1)
    for r in range(1, NUM_RANKS):
        lin[:, r] = nt + 1 + 40 * r + (np.arange(nt) * max(1, 40 - 2 * r)) // nt
    lin[:, 1:][rng.random((nt, NUM_RANKS - 1)) < 0.5] = 0
    lin[rng.random(nt) < 0.06, 0] = 0
    lin[rng.random(nt) < 0.04] = 0
    lin[: len(EDGE_WINDOWS)] = np.maximum(lin[: len(EDGE_WINDOWS)], 1)       # the border targets qualify on every rank
    lin[-len(EDGE_WINDOWS):] = np.maximum(lin[-len(EDGE_WINDOWS):], 1)
    return lin


class Table:
    """a context with announced windows and lineages, and the device side of the calls"""

    def __init__(self, windows, lin):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        cfg = api.default_config()
        h = C.c_void_p()
        assert api.lib().mc_create(C.byref(cfg), C.byref(h)) == 0, api.lib().mc_last_error(None)
        self.db = api.Database.from_handle(h.value, cfg)
        self.announce(windows, lin)

    def announce(self, windows, lin=None):
        self.windows = np.asarray(windows, dtype=np.uint32)
        self.db.load_target_windows(self.windows)
        if lin is not None:
            self.lin = lin
            self.db.set_lineages(lin)

    def to_device(self, cands):
        n, stride = cands.shape
        flat = np.ascontiguousarray(cands).view(np.uint32).reshape(n, stride * 4).view(np.int32)
        return self.torch.from_numpy(flat.copy()).to(self.dev) if n else self.torch.zeros((1, stride * 4), dtype=self.torch.int32, device=self.dev)

    def to_host(self, d, n, stride):
        return d[:n].cpu().numpy().view(np.uint32).view(api.cand_dtype).reshape(n, stride) if n else np.zeros((0, stride), dtype=api.cand_dtype)

    def add(self, cands, hitmin=0, lowest=0, stream=0):
        """marks on the device; the tensor is returned so that it outlives the asynchronous call"""
        d = self.to_device(cands)
        self.torch.cuda.synchronize()
        self.db.coverage_add_device(d.data_ptr(), cands.shape[0], cands.shape[1], hitmin=hitmin, lowest=lowest, stream=stream)
        return d

    def fresh(self, cands, hitmin=0, lowest=0):
        """an empty bitmap, one call, the counts"""
        self.db.coverage_counts(reset=True)
        d = self.add(cands, hitmin, lowest)
        covered, windows, st = self.db.coverage_counts()
        del d
        return covered, windows, st

    def check(self, cands, hitmin=0, lowest=0):
        covered, windows, st = self.fresh(cands, hitmin, lowest)
        want, outside, marked = coverage_ref.mark(self.windows, self.lin, cands, hitmin, lowest)
        assert np.array_equal(windows, self.windows)
        bad = np.flatnonzero(covered != want)
        assert bad.size == 0, (bad[:5], covered[bad[:5]], want[bad[:5]])
        assert (st["marked"], st["out_of_range"], st["bits"], st["calls"]) == (marked, outside, int(want.sum()), 1 if len(cands) else 0)
        return covered, st

    def close(self):
        self.db.close()


@pytest.fixture(scope="module")
def table():
    rng = np.random.default_rng(2024)
    nt = 300
    t = Table(make_windows(rng, nt), make_lineages(rng, nt))
    yield t
    t.close()


def rows_of(entries, stride):
    c = np.zeros((len(entries), stride), dtype=api.cand_dtype)
    for i, e in enumerate(entries):
        for j, x in enumerate(e if isinstance(e, list) else [e]):
            c[i, j] = x
    return c


def random_rows(rng, n, stride, windows, nt_lin):
    """ranges of 1 .. 3 windows (some longer, some reaching past their target), targets beyond both tables, rows that end early"""
    nt = len(windows)
    c = np.zeros((n, stride), dtype=api.cand_dtype)
    tgt = rng.integers(0, nt, size=(n, stride))
    tgt = np.where(rng.random((n, stride)) < 0.01, rng.choice(np.array([nt, nt_lin, nt_lin + 1, 2 ** 31, 2 ** 32 - 1]), size=(n, stride)), tgt)
    w = windows[np.minimum(tgt, nt - 1)].astype(np.int64)
    beg = (rng.random((n, stride)) * w).astype(np.int64)
    length = rng.integers(1, 4, size=(n, stride))
    length = np.where(rng.random((n, stride)) < 0.02, rng.integers(4, 200, size=(n, stride)), length)
    beg = np.where(rng.random((n, stride)) < 0.005, w + rng.integers(0, 3, size=(n, stride)), beg)          # beg beyond the target
    end = beg + length - 1
    end = np.where(rng.random((n, stride)) < 0.005, beg - 1, end)                                          # beg > end
    hits = rng.integers(1, 40, size=(n, stride))
    hits[rng.random((n, stride)) < 0.1] = 0                                                                # the row ends here, whatever follows
    c["tgt"] = tgt.astype(np.uint32); c["hits"] = hits.astype(np.uint32)
    c["beg"] = np.maximum(beg, 0).astype(np.uint32); c["end"] = np.maximum(end, 0).astype(np.uint32)
    return c


# ---- marking ---------------------------------------------------------------------------------------------------------------------------
def border_entries(windows):
    """(tgt, hits, beg, end) of every border case, each with hits 9"""
    last = len(windows) - 1
    e = []
    big = [t for t, w in enumerate(windows) if w >= 2048][0]
    e += [(big, 9, 3, 9), (big, 9, 30, 33), (big, 9, 5, 100), (big, 9, 64, 64), (big, 9, 31, 31), (big, 9, 32, 32), (big, 9, 1000, 1100)]
    for t in list(range(len(EDGE_WINDOWS))) + list(range(last - len(EDGE_WINDOWS) + 1, last + 1)):     # window 0 and window windows - 1 of every border size
        w = int(windows[t])
        e += [(t, 9, 0, 0), (t, 9, w - 1, w - 1)]
    e += [(0, 9, 0, 0), (last, 9, 0, 0)]
    return e


def test_single_ranges_on_an_empty_bitmap(table):
    """one entry at a time, against the model and against the count one can see"""
    big = [t for t, w in enumerate(table.windows) if w >= 2048][0]
    for beg, end in ((3, 9), (30, 33), (5, 100), (64, 64), (0, 0), (31, 32), (0, 2047), (2047, 2047), (63, 64), (0, 31), (32, 63)):
        covered, st = table.check(rows_of([(big, 9, beg, end)], 1))
        assert covered[big] == end - beg + 1 and covered.sum() == end - beg + 1 and st["out_of_range"] == 0
    w = int(table.windows[big])
    covered, st = table.check(rows_of([(big, 9, w - 3, w + 40)], 1))                # end beyond the target: the part inside, counted once
    assert covered[big] == 3 and st == dict(marked=1, out_of_range=1, bits=3, calls=1)
    for entry in ((big, 9, w, w + 2), (big, 9, w + 5, w + 5), (big, 9, 7, 6), (big, 9, 2 ** 32 - 1, 0), (len(table.windows), 9, 0, 0), (2 ** 32 - 1, 9, 0, 0)):
        covered, st = table.check(rows_of([entry], 1))
        # a tgt beyond the lineage table has no taxon: it does not qualify and is not counted at all
        beyond_lineages = entry[0] >= len(table.lin)
        assert covered.sum() == 0 and st == dict(marked=0, out_of_range=0 if beyond_lineages else 1, bits=0, calls=1), entry


def test_a_target_beyond_the_windows_but_inside_the_lineages_is_out_of_range():
    rng = np.random.default_rng(3)
    lin = make_lineages(rng, 320)
    lin[300:] = np.maximum(lin[300:], 1)
    t = Table(make_windows(rng, 300), lin)
    try:
        covered, st = t.check(rows_of([(300, 9, 0, 0), (319, 9, 0, 1), (320, 9, 0, 0), (5, 9, 0, 0)], 1))
        assert st == dict(marked=1, out_of_range=2, bits=1, calls=1) and covered[5] == 1
    finally:
        t.close()


@pytest.mark.parametrize("stride", [1, 2, 4, 7])
def test_borders_at_every_place_of_a_row(table, stride):
    """every border entry at place k % stride of its row, behind entries that do not qualify (below hits_min: skipped, not an end)"""
    entries = border_entries(table.windows)
    low = (20, 2, 0, 0)                                                              # 2 hits: below hits_min 5
    rows = []
    for k, e in enumerate(entries):
        rows.append([low] * (k % stride) + [e])
    c = rows_of(rows, stride)
    covered, st = table.check(c, hitmin=5)
    assert st["marked"] == len(entries) and covered[20] == 0
    covered0, st0 = table.check(c, hitmin=0)                                         # now the fillers mark target 20
    assert covered0[20] == (1 if stride > 1 else 0)
    # the same entries all in one call with everything else: rows that end at hits == 0 in front of entries that would mark
    ended = rows_of([[(6, 9, 0, 0), (6, 0, 0, 0), (7, 9, 0, 5)][:stride]], stride)
    covered, st = table.check(ended)
    assert covered[6] == 1 and covered[7] == 0 and st["marked"] == 1


def test_entries_without_a_taxon_are_skipped(table):
    lin = table.lin
    no0 = [t for t in range(len(lin)) if lin[t, 0] == 0 and lin[t, 1:].any()]
    empty = [t for t in range(len(lin)) if not lin[t].any()]
    assert no0 and empty
    a, b = no0[0], empty[0]
    ok = 0
    c = rows_of([[(a, 9, 0, 0), (ok, 9, 0, 0)], [(b, 9, 0, 0), (ok, 9, 0, 0)]], 2)
    covered, st = table.check(c, lowest=0)                                           # lowest 0: slot 0 itself, which a lacks
    assert covered[a] == 0 and covered[b] == 0 and covered[ok] == 1 and st["marked"] == 2
    first = int(np.flatnonzero(lin[a])[0])                                           # a's first filled slot
    covered, st = table.check(c, lowest=first)
    assert covered[a] == 1 and covered[b] == 0
    gap = [t for t in range(len(lin)) if lin[t, 3] == 0 and lin[t, 4:].any()]        # a hole at the rank asked for, something above it
    top = [t for t in range(len(lin)) if lin[t, :20].any() and lin[t, 20] == 0]      # nothing at the top rank
    assert gap and top
    c = rows_of([[(gap[0], 9, 0, 0)], [(top[0], 9, 0, 0)]], 1)
    covered, st = table.check(c, lowest=3)
    assert covered[gap[0]] == 1
    covered, st = table.check(c, lowest=20)
    assert covered[top[0]] == 0


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, MAX_BLOCKS * BLOCK + 1])
def test_row_counts(table, n):
    """the last row is the only one that marks its window: a grid that forgets a row is seen"""
    big = [t for t, w in enumerate(table.windows) if w >= 2048][0]
    c = np.zeros((n, 1), dtype=api.cand_dtype)
    c["tgt"] = 5; c["hits"] = 3; c["beg"] = 0; c["end"] = 1
    if n:
        c[n - 1, 0] = (big, 3, 77, 77)
    covered, st = table.check(c)
    assert st["marked"] == n and covered[big] == (1 if n else 0) and covered[5] == (2 if n > 1 else 0)


def test_identical_rows(table):
    big = [t for t, w in enumerate(table.windows) if w >= 2048][0]
    c = np.zeros((100_000, 2), dtype=api.cand_dtype)
    c[:, 0] = (big, 9, 29, 70)
    c[:, 1] = (big, 8, 60, 97)
    covered, st = table.check(c)
    assert covered[big] == 97 - 29 + 1 and covered.sum() == covered[big] and st["marked"] == 200_000


@pytest.mark.parametrize("stride", [1, 2, 4, 7])
def test_random_rows_equal_the_model(table, stride):
    rng = np.random.default_rng(100 + stride)
    c = random_rows(rng, 1_000_000, stride, table.windows, len(table.lin))
    c["tgt"][: 500_000, 0] = rng.integers(0, 10, size=500_000)                      # half of the reads pile onto ten targets
    c["beg"][: 500_000, 0] %= 2; c["end"][: 500_000, 0] = c["beg"][: 500_000, 0] + 1
    covered, st = table.check(c, hitmin=30, lowest=0)                                # (a quarter of the entries: the bitmap stays far from full)
    assert st["out_of_range"] > 0 and 0.05 < covered.sum() / table.windows.sum() < 0.8
    table.check(c[:200_000], hitmin=0, lowest=4)


# ---- accumulation ----------------------------------------------------------------------------------------------------------------------
def test_calls_accumulate_on_any_stream_and_reset_clears(table):
    torch = table.torch
    rng = np.random.default_rng(9)
    parts = [random_rows(rng, 300_000, 2, table.windows, len(table.lin)) for _ in range(4)]
    union = np.concatenate(parts)
    want, outside, marked = coverage_ref.mark(table.windows, table.lin, union, 3, 0)
    table.db.coverage_counts(reset=True)
    streams = [torch.cuda.Stream(device=table.dev) for _ in range(2)]
    # the context's own stream twice, then two streams of the caller at the same time
    held = [table.add(parts[0], 3), table.add(parts[1], 3)]
    d2, d3 = table.to_device(parts[2]), table.to_device(parts[3])
    torch.cuda.synchronize()
    for rep in range(2):                                                             # (marking twice changes the statistics, not the bitmap)
        for d, s in ((d2, streams[0]), (d3, streams[1])):
            table.db.coverage_add_device(d.data_ptr(), 300_000, 2, hitmin=3, stream=s.cuda_stream)
    for s in streams:
        s.synchronize()
    covered, windows, st = table.db.coverage_counts()
    one = [coverage_ref.mark(table.windows, table.lin, p, 3, 0) for p in parts]
    assert np.array_equal(covered, want)
    assert st["calls"] == 6 and st["marked"] == one[0][2] + one[1][2] + 2 * (one[2][2] + one[3][2]) and st["bits"] == int(want.sum())
    assert st["out_of_range"] == one[0][1] + one[1][1] + 2 * (one[2][1] + one[3][1])
    again = table.db.coverage_counts(reset=True)                                     # reading twice gives the same; this one resets
    assert np.array_equal(again[0], want) and again[2] == st
    covered, windows, st = table.db.coverage_counts()
    assert not covered.any() and st == dict(marked=0, out_of_range=0, bits=0, calls=0)
    del held


def test_other_windows_or_lineages_drop_coverage_and_mask():
    rng = np.random.default_rng(11)
    w1, lin = make_windows(rng, 300), make_lineages(rng, 300)
    t = Table(w1, lin)
    try:
        c = random_rows(rng, 50_000, 2, w1, 300)
        t.check(c)
        t.db.coverage_set_keep(np.ones(300, dtype=np.uint8))
        assert np.array_equal(t.db.coverage_drop(c[:100]), coverage_ref.drop(c[:100], np.ones(300, dtype=np.uint8)))
        w2 = make_windows(rng, 200)
        t.announce(w2)                                                               # other windows, the same lineages
        covered, windows, st = t.db.coverage_counts()
        assert len(covered) == 200 and not covered.any() and np.array_equal(windows, w2) and st == dict(marked=0, out_of_range=0, bits=0, calls=0)
        out = np.zeros_like(c[:100])
        rc = api.lib().mc_coverage_drop(t.db.h, c.ctypes.data, 100, 2, api.COVERAGE_HOST, out.ctypes.data, None)
        assert rc == MC_ERR_STATE and b"mask" in api.lib().mc_last_error(t.db.h)
        c2 = random_rows(rng, 50_000, 2, w2, 300)
        t.check(c2)                                                                  # the new layout works
        t.db.coverage_set_keep(np.ones(200, dtype=np.uint8))
        t.announce(w2, make_lineages(rng, 250))                                      # other lineages
        covered, windows, st = t.db.coverage_counts()
        assert not covered.any() and st["calls"] == 0
        with pytest.raises(api.McError):
            t.db.coverage_drop(c2[:10])
        t.check(c2, lowest=2)
    finally:
        t.close()


def test_host_arrays_equal_the_device_path(table):
    """MC_COVERAGE_HOST stages 64 MB pieces: 2^20 rows of stride 4; one row more starts a second piece"""
    rng = np.random.default_rng(21)
    n = (64 << 20) // (4 * 16) + 1
    big = [t for t, w in enumerate(table.windows) if w >= 2048][0]
    c = random_rows(rng, n, 4, table.windows, len(table.lin))
    c["tgt"][c["tgt"] == big] = 0                                                    # only the last row marks this target
    c[n - 1, 0] = (big, 30, 2000, 2003)
    dev_covered, dev_st = table.check(c, hitmin=4)
    table.db.coverage_counts(reset=True)
    table.db.coverage_add(c, hitmin=4)
    covered, windows, st = table.db.coverage_counts()
    assert np.array_equal(covered, dev_covered) and st == dev_st and covered[big] == 4


def test_counting_whole_targets(table):
    """targets of 1, 63, 64 and 65 words, marked from their first to their last window"""
    targets = [t for t in range(len(EDGE_WINDOWS))]
    words = sorted({(int(table.windows[t]) + 31) // 32 for t in targets})
    assert words == [1, 2, 63, 64, 65]
    c = rows_of([(t, 9, 0, int(table.windows[t]) - 1) for t in targets], 1)
    covered, st = table.check(c)
    assert np.array_equal(covered[targets], table.windows[targets]) and covered.sum() == table.windows[targets].sum()


# ---- dropping --------------------------------------------------------------------------------------------------------------------------
def test_drop(table):
    torch = table.torch
    rng = np.random.default_rng(31)
    nt = len(table.windows)
    with_tails = random_rows(rng, 1_000_000, 4, table.windows, len(table.lin))
    all_kept = np.ones(2 ** 16, dtype=np.uint8)                                      # (longer than the tables: every tgt below 2^16 stays)
    table.db.coverage_set_keep(None)
    with pytest.raises(api.McError):
        table.db.coverage_drop(with_tails[:10])                                      # MC_ERR_STATE without a mask
    table.db.coverage_set_keep(all_kept)
    c = coverage_ref.drop(with_tails, all_kept)                                      # rows with zeros behind their end
    small = c[(c["tgt"] < 2 ** 16).all(axis=1)][:1000]
    assert np.array_equal(table.db.coverage_drop(small), small)                      # keep all: the input comes back
    # the top entry goes and the next one moves up; everything goes; a tgt beyond the mask goes
    mask = np.ones(nt, dtype=np.uint8); mask[5] = 0
    table.db.coverage_set_keep(mask)
    rows = rows_of([[(5, 9, 1, 2), (6, 8, 3, 4), (7, 7, 5, 6)], [(5, 9, 1, 2), (5, 8, 3, 4)], [(6, 9, 1, 2), (nt, 8, 0, 0), (2 ** 32 - 1, 7, 0, 0), (7, 6, 0, 1)],
                    [(6, 9, 1, 2), (6, 0, 0, 0), (7, 7, 5, 6)]], 4)
    got = table.db.coverage_drop(rows)
    assert got["tgt"].tolist() == [[6, 7, 0, 0], [0, 0, 0, 0], [6, 7, 0, 0], [6, 0, 0, 0]]
    assert got["hits"].tolist() == [[8, 7, 0, 0], [0, 0, 0, 0], [9, 6, 0, 0], [9, 0, 0, 0]]
    assert got["beg"].tolist() == [[3, 5, 0, 0], [0, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0]]
    assert np.array_equal(got, coverage_ref.drop(rows, mask))
    # 10^6 random rows, half of the targets kept: out of place, in place, and the host form
    mask = (rng.random(nt) < 0.5).astype(np.uint8)
    table.db.coverage_set_keep(mask)
    want = coverage_ref.drop(with_tails, mask)
    n, stride = with_tails.shape
    d_in = table.to_device(with_tails)
    d_out = torch.full_like(d_in, -1)
    torch.cuda.synchronize()
    table.db.coverage_drop_device(d_in.data_ptr(), n, stride, d_out.data_ptr())
    table.db.synchronize()
    assert np.array_equal(table.to_host(d_out, n, stride), want)
    assert np.array_equal(table.to_host(d_in, n, stride), with_tails)               # the input is left alone
    table.db.coverage_drop_device(d_in.data_ptr(), n, stride, d_in.data_ptr())
    table.db.synchronize()
    assert np.array_equal(table.to_host(d_in, n, stride), want)
    assert np.array_equal(table.db.coverage_drop(with_tails[:300_000]), want[:300_000])
    for s in (1, 7):
        rows = random_rows(rng, 10_000, s, table.windows, len(table.lin))
        assert np.array_equal(table.db.coverage_drop(rows), coverage_ref.drop(rows, mask))
    assert table.db.coverage_drop(np.zeros((0, 3), dtype=api.cand_dtype)).shape == (0, 3)


def test_drop_of_host_arrays_beyond_one_staged_piece(table):
    """MC_COVERAGE_HOST stages 64 MB pieces: 2^20 rows of stride 4; one row more starts a second piece, which goes to out + 2^20 rows"""
    torch = table.torch
    rng = np.random.default_rng(33)
    stride = 4
    n = (64 << 20) // (stride * 16) + 1
    nt = len(table.windows)
    c = random_rows(rng, n, stride, table.windows, len(table.lin))
    mask = (rng.random(nt) < 0.5).astype(np.uint8)
    kept = int(np.flatnonzero(mask)[0])
    c[n - 1] = rows_of([[(kept, 9, 1, 2), (int(np.flatnonzero(mask == 0)[0]), 8, 3, 4), (kept, 7, 5, 6)]], stride)[0]       # the second piece: its middle entry goes
    table.db.coverage_set_keep(mask)
    want = coverage_ref.drop(c, mask)
    assert want["hits"][n - 1].tolist() == [9, 7, 0, 0] and 0.2 < (want["hits"] > 0).sum() / (c["hits"] > 0).sum() < 0.8
    got = table.db.coverage_drop(c)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (bad.size, int(bad[0]), got[bad[0]], want[bad[0]])
    d_in = table.to_device(c)
    d_out = torch.full_like(d_in, -1)
    torch.cuda.synchronize()
    table.db.coverage_drop_device(d_in.data_ptr(), n, stride, d_out.data_ptr())
    table.db.synchronize()
    assert np.array_equal(table.to_host(d_out, n, stride), got)


# ---- end to end on the toy database ----------------------------------------------------------------------------------------------------
def read_fasta(path):
    reads, cur = [], None
    for line in open(path, "rb"):
        line = line.strip()
        if line.startswith(b">"):
            if cur is not None:
                reads.append(cur)
            cur = b""
        elif cur is not None:
            cur += line
    if cur is not None:
        reads.append(cur)
    return reads


def device_batch(db, reads, dev):
    import torch
    pad = [len(r) + (-len(r)) % 4 for r in reads]
    offs = np.concatenate([[0], np.cumsum(pad)]).astype(np.int64)
    buf = np.zeros(int(offs[-1]) + 16, dtype=np.uint8)
    for r, o in zip(reads, offs[:-1]):
        buf[o:o + len(r)] = np.frombuffer(r, dtype=np.uint8)
    qinfo = np.zeros((len(reads), 4), dtype=np.uint32)
    qinfo[:, 0] = offs[:-1]; qinfo[:, 1] = [len(r) for r in reads]; qinfo[:, 2] = offs[:-1]
    mw = np.array([db.max_windows_in_range(len(r)) for r in reads], dtype=np.int32)
    return (torch.from_numpy(buf).to(dev), torch.from_numpy(qinfo.view(np.int32)).to(dev), torch.from_numpy(mw).to(dev), int(offs[-1]))


@pytest.mark.parametrize("K,lowest,hitmin", [(2, 0, 0), (4, 0, 5), (3, 4, 2)])
def test_real_candidates_end_to_end(K, lowest, hitmin):
    import torch
    reads = [r for r in read_fasta(os.path.join(GOLDEN, "cli_reads.fa")) if len(r) > 0]
    db = api.Database.open(os.path.join(GOLDEN, "toy32"), max_candidates=K)
    try:
        lin = db.lineages()
        cands, _, _ = db.query(reads, lowest=lowest)
        _, windows, _ = db.coverage_counts(reset=True)
        assert len(windows) == db.n_targets and windows.all()
        want, outside, marked = coverage_ref.mark(windows, lin, cands, hitmin, lowest)
        assert outside == 0 and marked > 50 and (want > 0).sum() >= 2
        db.coverage_add(cands, hitmin=hitmin, lowest=lowest)
        covered, _, st = db.coverage_counts(reset=True)
        assert np.array_equal(covered, want) and st == dict(marked=marked, out_of_range=0, bits=int(want.sum()), calls=1)
        # behind the query on its stream, without a wait in between: the context's own pipe, then the second pipe on a stream of the caller
        dev = torch.device("cuda", 0)
        seq, qi, mw, nch = device_batch(db, reads, dev)
        side = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        for j, st_ in enumerate((0, side.cuda_stream)):
            r = db.query_device(seq.data_ptr(), qi.data_ptr(), len(reads), nch, max_win_ptr=mw.data_ptr(), lowest=lowest, second_pipe=bool(j), stream=st_)
            db.coverage_add_device(r.cands, len(reads), K, hitmin=hitmin, lowest=lowest, stream=st_)
        db.synchronize(); side.synchronize()
        covered, _, st = db.coverage_counts(reset=True)
        assert np.array_equal(covered, want) and st["marked"] == 2 * marked and st["calls"] == 2
        # the whole chain, for every read
        opt = dict(hitmin=hitmin, hitdiff=0.5, lowest=lowest, highest=19)
        dropped_somewhere = False
        for percentile in (0.0, 0.05, 30, 0.7):
            got = db.classify_by_coverage(reads, percentile=percentile, **opt)
            keep = coverage_ref.keep(want, windows, api.percentile_factor(percentile))
            left = coverage_ref.drop(cands, keep)
            model = classify_ref.vote_all(lin, left, hitmin, api.hitdiff_factor(0.5), lowest, 19)
            triples = np.stack([got["taxon"].astype(np.int64), got["rank"].astype(np.int64), got["voters"].astype(np.int64)], axis=1)
            assert np.array_equal(triples, model), percentile
            if percentile == 0.0:
                assert np.array_equal(keep != 0, want > 0)
            dropped_somewhere |= bool(keep.sum() < (want > 0).sum())
        assert dropped_somewhere
    finally:
        db.close()
