"""GPU: mc_format_matches (matches_kernel<false>, tile_scan_kernel, matches_kernel<true>) -- the all-hits column rendered on the device --
and mc_format_mappings_with (format_lengths_kernel<true>, format_write_kernel<true>), which puts it into the mapping lines.

  * against the model (tests/matches_ref.py, itself held to the reference's lines by test_matches_witness_cpu.py), byte for byte, with
    guard bytes round the output on every call: reads per call and list lengths around a wave's tile, around the threshold between a
    wave's lists and the block's (BLOCK_LIST) and three times it; runs that are single entries, whole lists, that cross one, two and
    three tile borders, end on a tile's last entry and on the next tile's first, in lists of both kinds; run lengths and windows at
    every digit border and on both sides of 2^31; empty table entries, targets beyond the table, an empty table; a capacity one byte
    short; two streams at once; the host form across staged pieces with one read larger than a piece;
  * the extra column with every flag combination, pieces of 0 .. 70 000 bytes (longer than an output window), -mapped-only reads whose
    pieces are skipped, and no extra column at all (= mc_format_mappings);
  * against the reference: query, vote, all-hits column and lines enqueued on one stream without a synchronisation in between, on
    cli_reads.fa against toy32 -- the lines of the golden cases allhits_sequence and everything_species."""
import gzip
import json
import os

import numpy as np
import pytest

import format_ref
import matches_ref
from metacache_amd import api

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NUM_RANKS = 21
TILE, BLOCK_TILE, BLOCK_LIST = 64, 256, 1024      # a wave's tile, the block's, and kMatchBlockList: a list of more entries is the block's
GUARD, FILL = 256, 0xA5
NUM_TARGETS, NUM_RESULT = 500, 3000
WIN = api.MATCHES_WINDOWS


def random_texts(rng, count, empty_share):
    alphabet = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789 _.:()-", dtype=np.uint8)
    lens = rng.integers(1, 40, count)
    long = rng.random(count) < 0.1
    lens[long] = rng.integers(40, 301, int(long.sum()))
    lens[1::97] = 300
    lens[rng.random(count) < empty_share] = 0
    return [alphabet[rng.integers(0, len(alphabet), int(l))].tobytes() for l in lens]


@pytest.fixture(scope="module")
def texts():
    t = random_texts(np.random.default_rng(23), NUM_TARGETS, 0.1)
    t[0], t[1], t[2] = b"T0", b"", b"x" * 300
    assert max(map(len, t)) == 300 and 20 < sum(1 for x in t if not x) < 100
    return t


@pytest.fixture(scope="module")
def tables():
    rng = np.random.default_rng(17)
    t = {api.TEXT_RESULT: random_texts(rng, NUM_RESULT, 0.02), api.TEXT_TARGET_RESULT: random_texts(rng, NUM_TARGETS, 0.02),
         api.TEXT_CANDIDATE: random_texts(rng, NUM_TARGETS, 0.1)}
    t[api.TEXT_RESULT][0] = b"--"
    return t


@pytest.fixture(scope="module")
def db(texts, tables):
    d = api.Database.open(os.path.join(GOLDEN, "toy32"), max_candidates=3)
    d.format_matches_set_text(texts)
    for which, strings in tables.items():
        d.format_set_text(which, strings)
    yield d
    d.close()


def lists_of(runs_per_read):
    """[[(tgt, win, length), ...] per read] -> (hits loc_dtype, hit_off uint64 [n + 1]); neighbouring runs must differ"""
    tgt, win, off = [], [], [0]
    for runs in runs_per_read:
        for a, b in zip(runs, runs[1:]):
            assert a[:2] != b[:2]
        for t, w, l in runs:
            tgt.append(np.full(l, t, dtype=np.uint32)); win.append(np.full(l, w, dtype=np.uint32))
        off.append(off[-1] + sum(l for _, _, l in runs))
    hits = np.zeros(off[-1], dtype=api.loc_dtype)
    if off[-1]:
        hits["tgt"], hits["win"] = np.concatenate(tgt), np.concatenate(win)
    return hits, np.array(off, dtype=np.uint64)


def random_runs(rng, length, max_run=3, targets=NUM_TARGETS, windows=200):
    """a list of `length` locations in runs of 1 .. max_run entries, targets ascending"""
    runs, left, t, w = [], length, 0, 0
    while left:
        l = int(min(left, rng.integers(1, max_run + 1)))
        if rng.random() < 0.2:
            t, w = min(t + int(rng.integers(1, 4)), targets - 1), int(rng.integers(0, windows))
        w += 1
        if runs and runs[-1][:2] == (t, w):
            w += 1
        runs.append((t, w, l))
        left -= l
    return runs


class OnDevice:
    """lists in device memory, the output between two guard zones"""

    def __init__(self, hits, hit_off, capacity):
        import torch
        dev = torch.device("cuda", 0)
        self.n, self.capacity = len(hit_off) - 1, capacity
        self.hits = torch.from_numpy(np.concatenate([hits.view(np.int64), np.zeros(1, dtype=np.int64)])).to(dev)
        self.hit_off = torch.from_numpy(hit_off.view(np.int64).copy()).to(dev)
        self.piece_off = torch.full((self.n + 1 + api.FORMAT_SCRATCH,), -1, dtype=torch.int64, device=dev)
        room = capacity + (-capacity) % 16
        self.out = torch.full((GUARD + room + GUARD,), FILL, dtype=torch.uint8, device=dev)
        assert self.out.data_ptr() % 16 == 0
        torch.cuda.synchronize()

    def enqueue(self, db, flags, stream=0, capacity=None):
        db.format_matches_device(self.hits.data_ptr(), self.hit_off.data_ptr(), self.n, flags=flags, out_ptr=self.out.data_ptr() + GUARD,
                                 out_capacity=self.capacity if capacity is None else capacity, piece_off_ptr=self.piece_off.data_ptr(), stream=stream)

    def result(self):
        return self.out.cpu().numpy(), self.piece_off[:self.n + 1].cpu().numpy().view(np.uint64)


def assert_equal_to_model(buf, off, want_bytes, want_off, what):
    """offsets, the bytes, and every byte outside [0, off[n]) as it was"""
    bad = np.flatnonzero(off != want_off)
    assert bad.size == 0, (what, "offsets", int(bad[0]), int(off[bad[0]]), int(want_off[bad[0]]))
    total = len(want_bytes)
    got = buf[GUARD:GUARD + total].tobytes()
    if got != want_bytes:
        at = next(i for i in range(total) if got[i] != want_bytes[i])
        read = int(np.searchsorted(want_off, at, side="right")) - 1
        raise AssertionError((what, "byte", at, "read", read, got[max(0, at - 40):at + 20], want_bytes[max(0, at - 40):at + 20]))
    assert (buf[:GUARD] == FILL).all() and (buf[GUARD + total:] == FILL).all(), (what, "a byte outside the pieces was written")


def check(db, texts, runs_per_read, what, forms=(True, False)):
    hits, hit_off = lists_of(runs_per_read)
    n = len(runs_per_read)
    for windows in forms:
        want_bytes, want_off, runs, beyond = matches_ref.format_all(hits, hit_off, texts, windows)
        before = db.format_matches_stats()
        d = OnDevice(hits, hit_off, len(want_bytes))
        d.enqueue(db, WIN if windows else 0)
        db.synchronize()
        buf, off = d.result()
        assert_equal_to_model(buf, off, want_bytes, want_off, (what, windows))
        after = db.format_matches_stats()
        assert [x - y for x, y in zip(after, before)] == [1 if n else 0, n, runs, len(want_bytes), beyond], (what, windows)
    return want_bytes


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_reads_per_call(db, texts, n):
    rng = np.random.default_rng(100 + n)
    lens = rng.integers(0, 200, n)
    lens[::7] = 0
    if n > 5:
        lens[3], lens[n - 1] = BLOCK_LIST + 40, BLOCK_LIST + 1       # the block's lists among the waves', the last read one of them
    check(db, texts, [random_runs(rng, int(l)) for l in lens], f"n = {n}")


@pytest.mark.parametrize("length", [0, 1, 63, 64, 65, 127, 128, 129, BLOCK_LIST, BLOCK_LIST + 1, 3 * BLOCK_LIST])
def test_list_lengths(db, texts, length):
    rng = np.random.default_rng(200 + length)
    reads = [random_runs(rng, length) for _ in range(3)] + [random_runs(rng, 10), random_runs(rng, length, max_run=1), random_runs(rng, 5)]
    check(db, texts, reads, f"length {length}")


def around(before, run, after, t=7):
    """a list: `before` distinct entries, one run of `run` entries, `after` distinct entries"""
    return [(t, 1000 + k, 1) for k in range(before)] + [(t + 1, 5, run)] + [(t + 2, 2000 + k, 1) for k in range(after)]


def test_runs_against_the_tile_borders(db, texts):
    reads = {"all distinct": [(3, k, 1) for k in range(200)],
             "all distinct, the block's": [(3, k, 1) for k in range(BLOCK_LIST + 5)],
             "one run of 200": [(4, 9, 200)],
             "one run, the block's": [(4, 9, BLOCK_LIST + 5)],
             "60 .. 70": around(60, 11, 20),
             "ends at 63": around(50, 14, 30),
             "ends at 64": around(50, 15, 30),
             "begins at 64": around(64, 10, 3),
             "130 over three tiles": around(60, 130, 10),
             "193": around(0, 193, 1),
             "193 from 63 on": around(63, 193, 0),
             "ends in one entry": around(10, 117, 1),
             "one entry": [(5, 5, 1)],
             "two tiles, one run each": [(5, 5, 64), (5, 6, 64)],
             "the block's: a run over a block tile's border": around(250, 12, BLOCK_LIST),
             "the block's: ends at 255": around(200, 56, BLOCK_LIST),
             "the block's: ends at 256": around(200, 57, BLOCK_LIST),
             "the block's: over three waves' tiles": around(BLOCK_TILE + 60, 130, BLOCK_LIST),
             "the block's: over three block tiles": around(200, 2 * BLOCK_TILE + 100, BLOCK_LIST),
             "the block's: ends in one entry": around(BLOCK_LIST, 300, 1),
             "the block's: ends with its run": around(BLOCK_LIST - 100, 700, 0)}
    for what, runs in reads.items():
        check(db, texts, [runs], what)
    check(db, texts, list(reads.values()), "all in one call")


@pytest.mark.parametrize("run", [9, 10, 99, 100, 999, 1000])
def test_run_lengths_at_the_digit_borders(db, texts, run):
    want = check(db, texts, [around(3, run, 2), around(70, run, 0), [(0, 1, run)], around(BLOCK_LIST, run, 5)], f"run {run}", forms=(True,))
    assert f"T0/1:{run},".encode() in want


def test_windows_at_the_digit_borders_and_beyond_int(db, texts):
    wins = [0, 9, 10, 99999, 100000, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1]
    want = check(db, texts, [[(0, w, 2) for w in wins], [(0, w, 1) for w in wins[::-1]] * 20], "windows", forms=(True,))
    assert want.startswith(b"T0/0:2,T0/9:2,T0/10:2,T0/99999:2,T0/100000:2,T0/2147483647:2,T0/-2147483648:2,T0/-1:2,")
    check(db, texts, [[(0, w, 2) for w in wins]], "windows, plain form", forms=(False,))


def test_table_entries_empty_long_and_missing(db, texts):
    rng = np.random.default_rng(9)
    empty = [t for t in range(NUM_TARGETS) if not texts[t]][:5]
    reads = [[(t, 3, 2) for t in [0] + empty + [2]],                                     # empty entries: nothing in the window form, ":2," in the plain one
             [(t, k, 1) for k, t in enumerate([NUM_TARGETS, 5, NUM_TARGETS + 1, 2 ** 32 - 1, 6, 2 ** 31])],
             [(NUM_TARGETS + 7, 1, 300)],                                                # a whole list beyond the table: an empty piece
             [(2, k, 1) for k in range(150)],                                            # 300-byte entries
             [(int(t), 1, int(rng.integers(1, 4))) for t in range(NUM_TARGETS)],         # every entry of the table, lengths 0 .. 300
             [(NUM_TARGETS + k % 3, k, 1) for k in range(BLOCK_LIST + 70)]]              # ... and the block's
    hits, hit_off = lists_of(reads)
    _, _, _, beyond = matches_ref.format_all(hits, hit_off, texts, True)
    assert beyond == 4 + 1 + BLOCK_LIST + 70
    want = check(db, texts, reads, "table")
    assert want.startswith(b"T0:2,:2,:2,:2,:2,:2," + b"x" * 300 + b":2,")


def test_an_empty_table(db, texts):
    rng = np.random.default_rng(10)
    reads = [random_runs(rng, l) for l in (5, 0, 300, BLOCK_LIST + 3)]
    db.format_matches_set_text([])
    try:
        hits, hit_off = lists_of(reads)
        assert matches_ref.format_all(hits, hit_off, [], True)[0] == b""
        check(db, [], reads, "empty table")
    finally:
        db.format_matches_set_text(texts)
    check(db, texts, reads, "the table again")


def test_one_byte_short_writes_nothing_and_still_says_how_much(db, texts):
    rng = np.random.default_rng(11)
    reads = [random_runs(rng, int(l)) for l in rng.integers(0, 300, 200)] + [random_runs(rng, BLOCK_LIST + 9)]
    hits, hit_off = lists_of(reads)
    want_bytes, want_off, _, _ = matches_ref.format_all(hits, hit_off, texts, True)
    total = len(want_bytes)
    d = OnDevice(hits, hit_off, total)
    before = db.format_matches_stats()
    d.enqueue(db, WIN, capacity=total - 1)
    db.synchronize()
    buf, off = d.result()
    assert (buf == FILL).all()
    assert np.array_equal(off, want_off) and int(off[-1]) == total
    assert [x - y for x, y in zip(db.format_matches_stats(), before)] == [1, 201, 0, 0, 0]
    d.enqueue(db, WIN, capacity=total)
    db.synchronize()
    assert_equal_to_model(*d.result(), want_bytes, want_off, "second call")
    # the host form says so with its result
    piece_off = np.zeros(202, dtype=np.uint64)
    out = np.full(total, FILL, dtype=np.uint8)
    args = lambda cap: (db.h, hits.ctypes.data, hit_off.ctypes.data, 201, WIN | api.FORMAT_HOST, out.ctypes.data, cap, piece_off.ctypes.data, None)
    assert api.lib().mc_format_matches(*args(total - 1)) == -3                # MC_ERR_NOMEM
    assert (out == FILL).all() and np.array_equal(piece_off, want_off)
    assert api.lib().mc_format_matches(*args(total)) == 0
    assert out.tobytes() == want_bytes


def test_two_streams_at_once(db, texts):
    import torch
    rng = np.random.default_rng(12)
    cases = [lists_of([random_runs(rng, int(l)) for l in rng.integers(0, 400, 600)] + [random_runs(rng, 2 * BLOCK_LIST + j)]) for j in range(2)]
    wants = [matches_ref.format_all(h, o, texts, j == 0) for j, (h, o) in enumerate(cases)]
    devs = [OnDevice(h, o, len(w[0])) for (h, o), w in zip(cases, wants)]
    streams = [torch.cuda.Stream(device=torch.device("cuda", 0)) for _ in range(2)]
    before = db.format_matches_stats()
    for _ in range(3):
        for j, (d, st) in enumerate(zip(devs, streams)):
            d.enqueue(db, WIN if j == 0 else 0, stream=st.cuda_stream)
    for st in streams:
        st.synchronize()
    for j, (d, w) in enumerate(zip(devs, wants)):
        assert_equal_to_model(*d.result(), w[0], w[1], f"stream {j}")
    got = [x - y for x, y in zip(db.format_matches_stats(), before)]
    assert got == [6, 6 * 601, 3 * (wants[0][2] + wants[1][2]), 3 * (len(wants[0][0]) + len(wants[1][0])), 3 * (wants[0][3] + wants[1][3])]


def test_host_form_across_staged_pieces(db, texts):
    rng = np.random.default_rng(13)
    lens = rng.integers(0, 120, 60)
    lens[20] = 900                                                            # alone larger than a piece of 500 locations
    lens[40:43] = 0
    hits, hit_off = lists_of([random_runs(rng, int(l)) for l in lens])
    want_bytes, want_off, _, _ = matches_ref.format_all(hits, hit_off, texts, True)
    whole, off = db.format_matches(hits, hit_off, flags=WIN)
    assert whole == want_bytes and np.array_equal(off, want_off)
    db.set_tuning("format_stage_hits", 500)
    try:
        # the pieces as the rule cuts them: whole reads, at most 500 locations, a longer read alone
        pieces, i = 0, 0
        while i < 60:
            e = i + 1
            while e < 60 and int(hit_off[e + 1] - hit_off[i]) <= 500:
                e += 1
            pieces, i = pieces + 1, e
        assert pieces >= 3
        db.timing(True); db.timing_reset()
        got, off = db.format_matches(hits, hit_off, flags=WIN)
        _, launches = db.timing_get("matches_write")
        db.timing(False)
        assert launches == 2 * pieces                                         # for the size and for the bytes
        assert got == want_bytes and np.array_equal(off, want_off)
        plain, off = db.format_matches(hits, hit_off)
        want = matches_ref.format_all(hits, hit_off, texts, False)
        assert plain == want[0] and np.array_equal(off, want[1])
    finally:
        db.set_tuning("format_stage_hits", 0)
    empty, off = db.format_matches(np.zeros(0, dtype=api.loc_dtype), np.zeros(1, dtype=np.uint64))
    assert empty == b"" and off.tolist() == [0]


# ---- the column in the lines: mc_format_mappings_with -----------------------------------------------------------------------------------
ALL = format_ref.QUERY_IDS | format_ref.TRUTH | format_ref.TOPHITS | format_ref.LOCATIONS


def random_case(rng, n, stride=3, flags=ALL, column=b"\t|\t"):
    c = np.zeros((n, stride), dtype=api.cand_dtype)
    c["tgt"] = rng.integers(0, NUM_TARGETS, c.shape)
    c["hits"] = rng.integers(1, 300, c.shape)
    c["beg"] = rng.integers(0, 100000, c.shape)
    c["end"] = c["beg"] + rng.integers(0, 5, c.shape)
    used = rng.integers(0, stride + 1, n)
    c["hits"][np.arange(stride)[None, :] >= used[:, None]] = 0
    a = np.zeros(n, dtype=api.assignment_dtype)
    a["taxon"] = rng.integers(0, NUM_RESULT, n)
    a["taxon"][rng.random(n) < 0.2] = 0
    a["rank"] = np.where(a["taxon"] == 0, NUM_RANKS, rng.integers(0, 20, n))
    names = [bytes(rng.integers(33, 127, int(l)).astype(np.uint8)) for l in rng.integers(1, 25, n)]
    return {"column": column, "flags": flags, "cands": c, "assigned": a, "names": names, "truth": rng.integers(0, NUM_RESULT, n).astype(np.uint32),
            "query_ids": None, "first_query_id": 1, "win_stride": 112, "win_len": 127}


def random_pieces(rng, n, lens=None):
    lens = rng.integers(0, 200, n) if lens is None else np.asarray(lens)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    return bytes(rng.integers(33, 127, int(off[-1])).astype(np.uint8)), off


class LinesOnDevice:
    def __init__(self, case, extra, extra_off, capacity):
        import torch
        dev = torch.device("cuda", 0)
        n, stride = case["cands"].shape
        self.n, self.stride, self.capacity = n, stride, capacity
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)
        self.cands, self.assigned, self.truth = up(case["cands"].reshape(-1), np.int32), up(case["assigned"], np.int64), up(case["truth"], np.int32)
        nbytes, noff = api.pack_strings(case["names"])
        self.names, self.name_off = up(np.frombuffer(nbytes + b"\0", dtype=np.uint8), np.uint8), up(noff, np.int64)
        self.extra = None if extra is None else up(np.frombuffer(b"\0" * 3 + extra + b"\0", dtype=np.uint8), np.uint8)   # (the pieces begin at an odd address)
        self.extra_off = None if extra is None else up(extra_off, np.int64)
        self.line_off = torch.full((n + 1 + api.FORMAT_SCRATCH,), -1, dtype=torch.int64, device=dev)
        room = capacity + (-capacity) % 16
        self.out = torch.full((GUARD + room + GUARD,), FILL, dtype=torch.uint8, device=dev)
        self.opt = api.format_options(case["column"], case["win_stride"], case["win_len"])
        self.flags, self.first = case["flags"], case["first_query_id"]
        torch.cuda.synchronize()

    def enqueue(self, db, with_extra=True):
        db.format_device(self.opt, self.cands.data_ptr(), self.stride, self.assigned.data_ptr(), self.names.data_ptr(), self.name_off.data_ptr(), self.n,
                         flags=self.flags, truth_ptr=self.truth.data_ptr(), first_query_id=self.first, out_ptr=self.out.data_ptr() + GUARD,
                         out_capacity=self.capacity, line_off_ptr=self.line_off.data_ptr(), with_extra=with_extra,
                         extra_ptr=0 if self.extra is None else self.extra.data_ptr() + 3, extra_off_ptr=0 if self.extra is None else self.extra_off.data_ptr())

    def result(self):
        return self.out.cpu().numpy(), self.line_off[:self.n + 1].cpu().numpy().view(np.uint64)


def check_lines(db, tables, case, extra, extra_off, what):
    want_bytes, want_off, lines, beyond = matches_ref.lines_all(extra=extra, extra_off=extra_off, result=tables[api.TEXT_RESULT],
                                                                target_result=tables[api.TEXT_TARGET_RESULT], cand_text=tables[api.TEXT_CANDIDATE], **case)
    before = db.format_stats()
    d = LinesOnDevice(case, extra, extra_off, len(want_bytes))
    d.enqueue(db)
    db.synchronize()
    buf, off = d.result()
    assert_equal_to_model(buf, off, want_bytes, want_off, what)
    n = len(case["names"])
    assert [x - y for x, y in zip(db.format_stats(), before)] == [1, n, lines, len(want_bytes), beyond], what
    return want_bytes, want_off


@pytest.mark.parametrize("flags", [0, format_ref.QUERY_IDS, format_ref.TRUTH, format_ref.TOPHITS, format_ref.LOCATIONS, format_ref.MAPPED_ONLY,
                                   ALL | format_ref.MAPPED_ONLY])
def test_extra_column_with_every_flag_and_pieces_longer_than_a_window(db, tables, flags):
    rng = np.random.default_rng(300 + flags)
    n = 300
    lens = rng.integers(0, 200, n)
    lens[[0, 1, 2, 3, 4, 5]] = [0, 1, 15, 16, 17, 300]
    lens[[40, 41, 100, 255, 256, 299]] = [32768, 40000, 70000, 33000, 5000, 70000]       # next to each other, at a chunk's end and beginning, last
    case = random_case(rng, n, flags=flags)
    case["assigned"]["taxon"][[41, 255, 299]] = [5, 6, 7]                                  # (long pieces that have a line under -mapped-only too)
    extra, extra_off = random_pieces(rng, n, lens)
    want_bytes, _ = check_lines(db, tables, case, extra, extra_off, f"flags {flags}")
    assert extra[int(extra_off[299]):] in want_bytes


def test_extra_column_with_more_reads_than_tiles_of_sixteen(db, tables):
    """with the extra column a tile is 16 reads until the workspace's 2 048 tiles are used up: 40 000 reads make tiles of 32"""
    rng = np.random.default_rng(33)
    n = 40000
    assert n > api.FORMAT_SCRATCH * 16
    case = random_case(rng, n, stride=2, flags=format_ref.QUERY_IDS | format_ref.TOPHITS)
    lens = rng.integers(0, 24, n)
    lens[[31, 32, 20000]] = [3000, 40000, 5000]
    extra, extra_off = random_pieces(rng, n, lens)
    check_lines(db, tables, case, extra, extra_off, "40 000 reads")


def test_mapped_only_skips_the_pieces_of_unclassified_reads(db, tables):
    rng = np.random.default_rng(31)
    n = 700
    case = random_case(rng, n, flags=ALL | format_ref.MAPPED_ONLY)
    extra, extra_off = random_pieces(rng, n, rng.integers(1, 400, n))                       # every read has a piece
    for classified in ("none", "first", "last", "some"):
        if classified != "some":
            case["assigned"]["taxon"][:] = 0
            case["assigned"]["rank"][:] = NUM_RANKS
        if classified in ("first", "last"):
            at = 0 if classified == "first" else n - 1
            case["assigned"]["taxon"][at], case["assigned"]["rank"][at] = 17, 4
        if classified == "some":
            case["assigned"]["taxon"][::3], case["assigned"]["rank"][::3] = 9, 6
        want_bytes, want_off = check_lines(db, tables, case, extra, extra_off, classified)
        assert want_bytes.count(b"\n") == {"none": 0, "first": 1, "last": 1, "some": 234}[classified]


def test_without_an_extra_column_it_is_mc_format_mappings(db, tables):
    rng = np.random.default_rng(32)
    case = random_case(rng, 600)
    want_bytes, want_off, _, _ = format_ref.format_all(result=tables[api.TEXT_RESULT], target_result=tables[api.TEXT_TARGET_RESULT],
                                                       cand_text=tables[api.TEXT_CANDIDATE], **case)
    got = []
    for with_extra in (True, False):                                          # mc_format_mappings_with(extra = NULL), mc_format_mappings
        d = LinesOnDevice(case, None, None, len(want_bytes))
        d.enqueue(db, with_extra=with_extra)
        db.synchronize()
        got.append(d.result())
        assert_equal_to_model(*got[-1], want_bytes, want_off, with_extra)
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    # the host forms: with pieces across three staged pieces of reads, and with none
    extra, extra_off = random_pieces(rng, 600)
    opt = api.format_options(case["column"], case["win_stride"], case["win_len"])
    kw = dict(flags=case["flags"], truth=case["truth"], first_query_id=1)
    want = matches_ref.lines_all(extra=extra, extra_off=extra_off, result=tables[api.TEXT_RESULT], target_result=tables[api.TEXT_TARGET_RESULT],
                                 cand_text=tables[api.TEXT_CANDIDATE], **case)
    db.set_tuning("format_stage_rows", 250)
    try:
        lines, off = db.format_mappings(opt, case["cands"], case["assigned"], case["names"], extra=extra, extra_off=extra_off, **kw)
        assert lines == want[0] and np.array_equal(off, want[1])
        lines, off = db.format_mappings(opt, case["cands"], case["assigned"], case["names"], **kw)
        assert lines == want_bytes and np.array_equal(off, want_off)
    finally:
        db.set_tuning("format_stage_rows", 0)


# ---- the chain, against the reference ------------------------------------------------------------------------------------------------
def cli_case(name):
    with gzip.open(os.path.join(GOLDEN, "cli_expected.json.gz"), "rt") as f:
        return json.load(f)[name]


def read_fasta(path):
    recs = []
    with open(path, "rb") as f:
        for line in f.read().split(b"\n"):
            if line.startswith(b">"):
                recs.append([line[1:].split(b" ")[0], b""])
            elif line.strip():
                recs[-1][1] += line.strip()
    return [(h, s, i + 1) for i, (h, s) in enumerate(recs) if s]           # (a record without a sequence has an id and no line)


@pytest.mark.parametrize("case,maxcand,lowest,flags,text_kw", [("allhits_sequence", 3, 0, api.FORMAT_TOPHITS, {}),
                                                               ("everything_species", 2, 4, api.FORMAT_QUERY_IDS | api.FORMAT_TOPHITS, {"lowest": 4, "lineage": True, "taxids": True})])
def test_query_vote_column_and_lines_on_one_stream_print_the_reference_lines(case, maxcand, lowest, flags, text_kw):
    import torch
    rec = cli_case(case)
    assert "-allhits" in rec["args"]
    golden = "".join(l + "\n" for l in rec["lines"] if l and not l.startswith("#")).encode()
    column_at = 2 if flags & api.FORMAT_QUERY_IDS else 1
    column_bytes = sum(len(l.split("\t|\t")[column_at]) for l in rec["lines"] if l and not l.startswith("#"))
    recs = read_fasta(os.path.join(GOLDEN, "cli_reads.fa"))
    reads = [s for _, s, _ in recs]
    dev = torch.device("cuda", 0)
    d = api.Database.open(os.path.join(GOLDEN, "toy32"), max_candidates=maxcand)
    try:
        taxa, target_lin = d.taxa(), d.lineages()
        for which, strings in api.mapping_texts(taxa, d.taxon_table()[0], target_lin, **text_kw).items():
            d.format_set_text(which, strings)
        d.format_matches_set_text(api.match_texts(taxa, target_lin, lowest))
        n = len(reads)
        pad = [len(r) + (-len(r)) % 4 for r in reads]
        offs = np.concatenate([[0], np.cumsum(pad)]).astype(np.int64)
        buf = np.zeros(int(offs[-1]) + 16, dtype=np.uint8)
        for r, o in zip(reads, offs[:-1]):
            buf[o:o + len(r)] = np.frombuffer(r, dtype=np.uint8)
        qinfo = np.zeros((n, 4), dtype=np.uint32)
        qinfo[:, 0] = offs[:-1]; qinfo[:, 1] = [len(r) for r in reads]; qinfo[:, 2] = offs[:-1]
        mw = np.array([d.max_windows_in_range(len(r)) for r in reads], dtype=np.int32)
        seq, qi, dmw = torch.from_numpy(buf).to(dev), torch.from_numpy(qinfo.view(np.int32)).to(dev), torch.from_numpy(mw).to(dev)
        nbytes, noff = api.pack_strings([h for h, _, _ in recs])
        ids = torch.from_numpy(np.array([i for _, _, i in recs], dtype=np.int64)).to(dev)
        names = torch.from_numpy(np.frombuffer(nbytes, dtype=np.uint8).copy()).to(dev)
        name_off = torch.from_numpy(noff.view(np.int64)).to(dev)
        assigned = torch.empty(n, dtype=torch.int64, device=dev)
        column_cap = column_bytes + (-column_bytes) % 16
        pieces = torch.full((column_cap,), FILL, dtype=torch.uint8, device=dev)
        piece_off = torch.empty(n + 1 + api.FORMAT_SCRATCH, dtype=torch.int64, device=dev)
        capacity = len(golden) + 100
        out = torch.full((capacity,), FILL, dtype=torch.uint8, device=dev)
        line_off = torch.empty(n + 1 + api.FORMAT_SCRATCH, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        # the golden cases' headers: hit threshold 5, ranks up to domain, the default -hitdiff
        r = d.query_device(seq.data_ptr(), qi.data_ptr(), n, int(offs[-1]), max_win_ptr=dmw.data_ptr(), lowest=lowest, want_allhits=True)
        d.classify_device(r.cands, n, maxcand, out_ptr=assigned.data_ptr(), hitmin=5, hitdiff=1.0, lowest=lowest, highest=19)
        d.format_matches_device(r.hits, r.hit_offsets, n, flags=api.MATCHES_WINDOWS if lowest == 0 else 0, out_ptr=pieces.data_ptr(),
                                out_capacity=column_cap, piece_off_ptr=piece_off.data_ptr())
        d.format_device(api.format_options(b"\t|\t", d.stride, d.w), r.cands, maxcand, assigned.data_ptr(), names.data_ptr(), name_off.data_ptr(), n,
                        flags=flags, query_ids_ptr=ids.data_ptr(), out_ptr=out.data_ptr(), out_capacity=capacity, line_off_ptr=line_off.data_ptr(),
                        extra_ptr=pieces.data_ptr(), extra_off_ptr=piece_off.data_ptr())
        d.synchronize()
        off = line_off[:n + 1].cpu().numpy()
        got = out.cpu().numpy()
        assert n == 399 and int(piece_off[n].item()) == column_bytes and int(off[-1]) == len(golden)
        assert got[:len(golden)].tobytes() == golden and (got[len(golden):] == FILL).all()
        assert (pieces.cpu().numpy()[column_bytes:] == FILL).all()
        assert d.format_stats() == [1, 399, 399, len(golden), 0]
        st = d.format_matches_stats()
        runs = sum(l.split("\t|\t")[column_at].count(",") for l in rec["lines"] if l and not l.startswith("#"))      # (every run ends in its comma)
        assert st == [1, 399, runs, column_bytes, 0] and runs > 399
    finally:
        d.close()
