"""GPU: mc_format_mappings (format_lengths_kernel, tile_scan_kernel, format_write_kernel) -- the mapping lines rendered on the device.

  * against the model (tests/format_ref.py, itself held to the reference's lines by test_format_witness_cpu.py): bytes and offsets, on
    synthetic tables of about 3 000 result texts and 500 targets (text lengths 0 .. 300, some candidate texts empty); the sizes around
    a wave and a block, one beyond the scan block's tile, one that makes a tile longer than a block; numbers at every digit border;
    names of length 0 .. 5 000 (one of them among short ones: the line that spans output windows); strides, full and empty lists,
    indices beyond their tables, column separators of 0 .. 16 bytes, every flag alone and all together, -mapped-only with no, the first
    and the last read classified, sequence-level results with and without the targets' table; guard bytes around the output on EVERY
    call; a capacity one byte short; two streams at once; the host form across three staged pieces;
  * against the reference: query, vote and formatting enqueued on one stream without a synchronisation in between, on cli_reads.fa
    against toy32 -- the lines of the golden case hitdiff_percent."""
import gzip
import json
import os

import numpy as np
import pytest

import format_ref
from metacache_amd import api

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NUM_RANKS = 21
SCAN_TILE, MAX_TILES, BLOCK = 256, api.FORMAT_SCRATCH, 256     # tile_scan_kernel scans 256 tile sums per trip; at most MAX_TILES tiles, of whole blocks of reads
GUARD, FILL = 256, 0xA5
ALL = format_ref.QUERY_IDS | format_ref.TRUTH | format_ref.TOPHITS | format_ref.LOCATIONS
NUM_RESULT, NUM_TARGETS = 3000, 500


def random_texts(rng, count, empty_share):
    alphabet = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789 _.:()-", dtype=np.uint8)
    lens = rng.integers(1, 60, count)
    long = rng.random(count) < 0.1
    lens[long] = rng.integers(60, 301, int(long.sum()))
    lens[1::97] = 300
    lens[rng.random(count) < empty_share] = 0
    return [alphabet[rng.integers(0, len(alphabet), int(l))].tobytes() for l in lens]


@pytest.fixture(scope="module")
def tables():
    rng = np.random.default_rng(17)
    t = {api.TEXT_RESULT: random_texts(rng, NUM_RESULT, 0.02), api.TEXT_TARGET_RESULT: random_texts(rng, NUM_TARGETS, 0.02),
         api.TEXT_CANDIDATE: random_texts(rng, NUM_TARGETS, 0.1)}
    t[api.TEXT_RESULT][0] = b"--"
    assert max(map(len, t[api.TEXT_RESULT])) == 300 and min(map(len, t[api.TEXT_RESULT])) == 0
    assert 20 < sum(1 for x in t[api.TEXT_CANDIDATE] if not x) < 100
    return t


@pytest.fixture(scope="module")
def db(tables):
    d = api.Database.open(os.path.join(GOLDEN, "toy32"), max_candidates=3)
    for which, strings in tables.items():
        d.format_set_text(which, strings)
    yield d
    d.close()


def random_case(rng, n, stride=2, flags=ALL, column=b"\t|\t", name_len=(1, 24)):
    """n reads: lists of random length (full ones and empty ones among them), taxa and targets mostly inside their tables"""
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
    a["voters"] = rng.integers(0, 5, n)
    names = [bytes(rng.integers(33, 127, int(l)).astype(np.uint8)) for l in rng.integers(name_len[0], name_len[1] + 1, n)]
    return {"column": column, "flags": flags, "cands": c, "assigned": a, "names": names, "truth": rng.integers(0, NUM_RESULT, n).astype(np.uint32),
            "query_ids": None, "first_query_id": 1, "win_stride": 112, "win_len": 127}


def model(tables, case, target_result=True):
    return format_ref.format_all(result=tables[api.TEXT_RESULT], target_result=tables[api.TEXT_TARGET_RESULT] if target_result else None,
                                 cand_text=tables[api.TEXT_CANDIDATE], **case)


class OnDevice:
    """a case's arrays in device memory, the output between two guard zones"""

    def __init__(self, case, capacity, packed_names=None):
        import torch
        dev = torch.device("cuda", 0)
        n, stride = case["cands"].shape
        self.n, self.stride, self.capacity = n, stride, capacity
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(dev)
        self.cands = up(case["cands"].reshape(-1), np.int32) if n else torch.zeros(4, dtype=torch.int32, device=dev)
        self.assigned = up(case["assigned"], np.int64) if n else torch.zeros(1, dtype=torch.int64, device=dev)
        self.truth = up(case["truth"], np.int32) if n else torch.zeros(1, dtype=torch.int32, device=dev)
        self.ids = None if case["query_ids"] is None else up(np.asarray(case["query_ids"], dtype=np.uint64), np.int64)
        nbytes, noff = packed_names if packed_names is not None else api.pack_strings(case["names"])
        self.names = up(np.frombuffer(nbytes + b"\0", dtype=np.uint8), np.uint8)
        self.name_off = up(noff, np.int64)
        self.line_off = torch.full((n + 1 + api.FORMAT_SCRATCH,), -1, dtype=torch.int64, device=dev)
        room = capacity + (-capacity) % 16
        self.out = torch.full((GUARD + room + GUARD,), FILL, dtype=torch.uint8, device=dev)
        assert self.out.data_ptr() % 16 == 0
        self.opt = api.format_options(case["column"], case["win_stride"], case["win_len"])
        self.flags, self.first = case["flags"], case["first_query_id"]
        torch.cuda.synchronize()

    def enqueue(self, db, stream=0, capacity=None):
        db.format_device(self.opt, self.cands.data_ptr(), self.stride, self.assigned.data_ptr(), self.names.data_ptr(), self.name_off.data_ptr(), self.n,
                         flags=self.flags, truth_ptr=self.truth.data_ptr(), query_ids_ptr=0 if self.ids is None else self.ids.data_ptr(),
                         first_query_id=self.first, out_ptr=self.out.data_ptr() + GUARD, out_capacity=self.capacity if capacity is None else capacity,
                         line_off_ptr=self.line_off.data_ptr(), stream=stream)

    def result(self):
        """(bytes of the whole buffer, line_off [n + 1])"""
        return self.out.cpu().numpy(), self.line_off[:self.n + 1].cpu().numpy().view(np.uint64)


def assert_equal_to_model(buf, off, want_bytes, want_off, what):
    """offsets, the bytes, and every byte outside [0, line_off[n]) as it was"""
    bad = np.flatnonzero(off != want_off)
    assert bad.size == 0, (what, "line_off", int(bad[0]), int(off[bad[0]]), int(want_off[bad[0]]))
    total = len(want_bytes)
    got = buf[GUARD:GUARD + total].tobytes()
    if got != want_bytes:
        at = next(i for i in range(total) if got[i] != want_bytes[i])
        line = int(np.searchsorted(want_off, at, side="right")) - 1
        raise AssertionError((what, "byte", at, "line", line, got[max(0, at - 40):at + 20], want_bytes[max(0, at - 40):at + 20]))
    assert (buf[:GUARD] == FILL).all() and (buf[GUARD + total:] == FILL).all(), (what, "a byte outside the lines was written")


def check(db, tables, case, what, target_result=True):
    want_bytes, want_off, lines, beyond = model(tables, case, target_result)
    before = db.format_stats()
    d = OnDevice(case, len(want_bytes))
    d.enqueue(db)
    db.synchronize()
    buf, off = d.result()
    assert_equal_to_model(buf, off, want_bytes, want_off, what)
    after = db.format_stats()
    n = len(case["names"])
    assert [x - y for x, y in zip(after, before)] == [1 if n else 0, n, lines, len(want_bytes), beyond], what     # (a call without reads is not counted)
    return want_bytes, want_off


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_sizes_around_a_wave_and_a_block(db, tables, n):
    check(db, tables, random_case(np.random.default_rng(100 + n), n), f"n = {n}")


@pytest.mark.parametrize("n", [SCAN_TILE * BLOCK + 1, MAX_TILES * BLOCK + 300])
def test_more_tiles_than_a_scan_trip_and_tiles_longer_than_a_block(db, tables, n):
    """the first size has 257 tiles (the scan block's second trip carries the first's sum), the second makes tiles of two chunks;
    the reads repeat a pattern of 1 000, so the model renders each distinct line once"""
    rng = np.random.default_rng(n)
    period = 1000
    p = random_case(rng, period, stride=2, flags=ALL)
    p["query_ids"] = rng.integers(0, 2 ** 63, period).astype(np.uint64)
    pb, po, plines, pbeyond = model(tables, p)
    reps, rest = divmod(n, period)
    def tiled_offsets(offsets):
        lens, out = np.diff(offsets), np.zeros(n + 1, dtype=np.uint64)
        out[1:] = np.cumsum(np.concatenate([np.tile(lens, reps), lens[:rest]]), dtype=np.uint64)
        return out

    want_off = tiled_offsets(po)
    want_bytes = pb * reps + pb[:int(po[rest])]
    idx = np.arange(n) % period
    case = dict(p, cands=p["cands"][idx], assigned=p["assigned"][idx], truth=p["truth"][idx], query_ids=p["query_ids"][idx])
    nbytes, noff = api.pack_strings(p["names"])
    packed = (nbytes * reps + nbytes[:int(noff[rest])], tiled_offsets(noff))
    d = OnDevice(case, len(want_bytes), packed_names=packed)
    d.enqueue(db)
    db.synchronize()
    buf, off = d.result()
    assert_equal_to_model(buf, off, want_bytes, want_off, f"n = {n}")


BORDERS = sorted({0, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1} | {10 ** k - 1 for k in range(1, 20)} | {10 ** k for k in range(1, 20)})


def test_numbers_at_every_digit_border(db, tables):
    rng = np.random.default_rng(5)
    # the ids as an array ...
    case = random_case(rng, len(BORDERS), stride=2)
    case["query_ids"] = np.array(BORDERS, dtype=np.uint64)
    check(db, tables, case, "id array")
    # ... and as first_query_id + i, around every border (2^64 - 1 is followed by 0)
    for b in BORDERS:
        case = random_case(rng, 3, stride=1, flags=format_ref.QUERY_IDS)
        case["first_query_id"] = (b - 1) % 2 ** 64
        want_bytes, _ = check(db, tables, case, f"first_query_id {b} - 1")
        assert want_bytes.split(b"\n")[1].startswith(str(b).encode() + b"\t|\t")
    # hits, and window ranges whose products with the stride pass 2^32
    hits = [1, 9, 10, 99, 100, 65535, 2 ** 32 - 1]
    case = random_case(rng, len(hits), stride=2, flags=format_ref.TOPHITS | format_ref.LOCATIONS)
    case["cands"]["hits"][:, 0] = hits
    case["cands"]["hits"][:, 1] = hits[::-1]
    case["cands"]["tgt"][:, 0] = [t for t in range(NUM_TARGETS) if tables[api.TEXT_CANDIDATE][t]][:len(hits)]
    case["cands"]["beg"][:, 0] = [0, 1, 2 ** 32 // 112, 2 ** 32 // 112 + 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1]
    case["cands"]["end"][:, 0] = [0, 2 ** 32 // 112, 2 ** 32 // 112 + 1, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1]
    case["win_stride"], case["win_len"] = 112, 2 ** 32 - 1
    want_bytes, _ = check(db, tables, case, "hits and locations")
    assert b":4294967295" in want_bytes and str(112 * (2 ** 32 - 1) + 2 ** 32 - 1).encode() in want_bytes
    case["win_stride"], case["win_len"] = 2 ** 32 - 1, 0
    check(db, tables, case, "the largest stride")


def test_names_of_every_length_and_one_line_that_spans_windows(db, tables):
    rng = np.random.default_rng(6)
    lens = [0, 1, 15, 16, 17, 255, 5000]
    case = random_case(rng, len(lens))
    case["names"] = [bytes(rng.integers(33, 127, l).astype(np.uint8)) for l in lens]
    check(db, tables, case, "name lengths")
    # one 5 000-byte name among short ones, at the beginning, in the middle of a chunk, at its end and in the next one
    for where in (0, 100, 255, 256, 299):
        case = random_case(rng, 300)
        case["names"][where] = bytes(rng.integers(33, 127, 5000).astype(np.uint8))
        check(db, tables, case, f"long name at {where}")
    # lines longer than an output window of 32 KiB, next to each other
    case = random_case(rng, 40)
    for where, l in ((3, 40000), (4, 70000), (5, 32768), (39, 33000)):
        case["names"][where] = bytes(rng.integers(33, 127, l).astype(np.uint8))
    check(db, tables, case, "names longer than a window")


@pytest.mark.parametrize("stride", [1, 2, 4, 8])
def test_strides_full_lists_and_empty_lists(db, tables, stride):
    rng = np.random.default_rng(70 + stride)
    case = random_case(rng, 500, stride=stride)
    case["cands"]["hits"][:100] = rng.integers(1, 50, (100, stride))          # full lists: no terminator
    case["cands"]["hits"][100:200] = 0                                        # empty lists
    case["cands"]["hits"][200:220, 0] = 0                                     # ... whose later entries are not looked at
    check(db, tables, case, f"stride {stride}")


def test_indices_beyond_their_tables(db, tables):
    rng = np.random.default_rng(8)
    case = random_case(rng, 400, stride=3)
    case["cands"]["tgt"][::5, 1] = [NUM_TARGETS, NUM_TARGETS + 1, 2 ** 32 - 1, 2 ** 31] * 20
    case["assigned"]["taxon"][::7] = NUM_RESULT
    case["assigned"]["taxon"][1::7] = 2 ** 32 - 1
    case["truth"][::3] = NUM_RESULT + 5
    case["assigned"]["rank"][2::9] = 0                                        # sequence level ...
    case["assigned"]["taxon"][2::9] = 5
    case["cands"]["tgt"][2::9, 0] = NUM_TARGETS + 3                            # ... with a first candidate that is no target
    _, _, _, beyond = model(tables, case)
    assert beyond > 200
    check(db, tables, case, "beyond the tables")


@pytest.mark.parametrize("column", [b"", b"\t", b"/%/", b"0123456789abcdef"])
def test_column_separators(db, tables, column):
    check(db, tables, random_case(np.random.default_rng(len(column)), 300, column=column), f"column {column!r}")


@pytest.mark.parametrize("flags", [0, format_ref.QUERY_IDS, format_ref.TRUTH, format_ref.TOPHITS, format_ref.LOCATIONS, format_ref.MAPPED_ONLY,
                                   ALL | format_ref.MAPPED_ONLY])
def test_every_flag_alone_and_all_together(db, tables, flags):
    check(db, tables, random_case(np.random.default_rng(flags), 300, stride=3, flags=flags), f"flags {flags}")


@pytest.mark.parametrize("classified", ["none", "first", "last"])
def test_mapped_only_with_few_lines(db, tables, classified):
    case = random_case(np.random.default_rng(9), 700, flags=ALL | format_ref.MAPPED_ONLY)
    case["assigned"]["taxon"] = 0
    case["assigned"]["rank"] = NUM_RANKS
    if classified != "none":
        at = 0 if classified == "first" else 699
        case["assigned"]["taxon"][at], case["assigned"]["rank"][at] = 17, 4
    want_bytes, want_off = check(db, tables, case, classified)
    assert want_bytes.count(b"\n") == (0 if classified == "none" else 1) and int(want_off[-1]) == len(want_bytes)


def test_sequence_level_results_with_and_without_the_targets_table(db, tables):
    case = random_case(np.random.default_rng(10), 400, flags=0)
    case["assigned"]["taxon"][case["assigned"]["taxon"] == 0] = 1
    case["assigned"]["rank"][::2] = 0
    with_table, _ = check(db, tables, case, "with the table")
    db.format_set_text(api.TEXT_TARGET_RESULT, [])                            # an empty table is none
    try:
        without, _ = check(db, tables, case, "without the table", target_result=False)
    finally:
        db.format_set_text(api.TEXT_TARGET_RESULT, tables[api.TEXT_TARGET_RESULT])
    assert with_table != without
    check(db, tables, case, "the table again")


def test_one_byte_short_writes_nothing_and_still_says_how_much(db, tables):
    case = random_case(np.random.default_rng(11), 1000)
    want_bytes, want_off, _, _ = model(tables, case)
    total = len(want_bytes)
    d = OnDevice(case, total)
    before = db.format_stats()
    d.enqueue(db, capacity=total - 1)
    db.synchronize()
    buf, off = d.result()
    assert (buf == FILL).all()
    assert np.array_equal(off, want_off) and int(off[-1]) == total
    assert [x - y for x, y in zip(db.format_stats(), before)] == [1, 1000, 0, 0, 0]
    d.enqueue(db, capacity=total)
    db.synchronize()
    assert_equal_to_model(*d.result(), want_bytes, want_off, "second call")
    # the host form says so with its result
    line_off = np.zeros(1001, dtype=np.uint64)
    out = np.full(total, FILL, dtype=np.uint8)
    nbytes, noff = api.pack_strings(case["names"])
    nbuf = np.frombuffer(nbytes, dtype=np.uint8)
    args = lambda cap: (db.h, api.format_options(case["column"], case["win_stride"], case["win_len"]), case["cands"].ctypes.data, 2, case["assigned"].ctypes.data,
                        case["truth"].ctypes.data, None, 1, nbuf.ctypes.data, noff.ctypes.data, 1000, case["flags"] | api.FORMAT_HOST, out.ctypes.data, cap,
                        line_off.ctypes.data, None)
    assert api.lib().mc_format_mappings(*args(total - 1)) == -3               # MC_ERR_NOMEM
    assert (out == FILL).all() and np.array_equal(line_off, want_off)
    assert api.lib().mc_format_mappings(*args(total)) == 0
    assert out.tobytes() == want_bytes


def test_two_streams_at_once(db, tables):
    import torch
    cases = [random_case(np.random.default_rng(20 + j), 20000, stride=2 + j) for j in range(2)]
    wants = [model(tables, c) for c in cases]
    devs = [OnDevice(c, len(w[0])) for c, w in zip(cases, wants)]
    streams = [torch.cuda.Stream(device=torch.device("cuda", 0)) for _ in range(2)]
    before = db.format_stats()
    for _ in range(3):
        for d, st in zip(devs, streams):
            d.enqueue(db, stream=st.cuda_stream)
    for st in streams:
        st.synchronize()
    for j, (d, w) in enumerate(zip(devs, wants)):
        assert_equal_to_model(*d.result(), w[0], w[1], f"stream {j}")
    got = [x - y for x, y in zip(db.format_stats(), before)]
    assert got == [6, 6 * 20000, 3 * (wants[0][2] + wants[1][2]), 3 * (len(wants[0][0]) + len(wants[1][0])), 3 * (wants[0][3] + wants[1][3])]


def test_host_form_across_three_pieces(db, tables):
    rng = np.random.default_rng(31)
    case = random_case(rng, 1000, stride=3)
    case["query_ids"] = rng.integers(0, 2 ** 64, 1000, dtype=np.uint64)
    case["names"][450] = bytes(rng.integers(33, 127, 5000).astype(np.uint8))
    want_bytes, want_off, _, _ = model(tables, case)
    opt = api.format_options(case["column"], case["win_stride"], case["win_len"])
    kw = dict(flags=case["flags"], truth=case["truth"], query_ids=case["query_ids"])
    whole, off = db.format_mappings(opt, case["cands"], case["assigned"], case["names"], **kw)
    assert whole == want_bytes and np.array_equal(off, want_off)
    db.set_tuning("format_stage_rows", 400)
    try:
        db.timing(True); db.timing_reset()
        got, off = db.format_mappings(opt, case["cands"], case["assigned"], case["names"], **kw)
        _, launches = db.timing_get("format_write")
        db.timing(False)
        assert launches == 6                                                  # 400 + 400 + 200, for the size and for the bytes
        assert got == want_bytes and np.array_equal(off, want_off)
        case["query_ids"] = None
        got, off = db.format_mappings(opt, case["cands"], case["assigned"], case["names"], flags=case["flags"], truth=case["truth"], first_query_id=2 ** 64 - 500)
        want = model(tables, dict(case, first_query_id=2 ** 64 - 500))
        assert got == want[0] and np.array_equal(off, want[1])
    finally:
        db.set_tuning("format_stage_rows", 0)
    empty, off = db.format_mappings(opt, np.zeros((0, 2), dtype=api.cand_dtype), np.zeros(0, dtype=api.assignment_dtype), [])
    assert empty == b"" and off.tolist() == [0]


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


def test_query_vote_and_format_on_one_stream_print_the_reference_lines():
    import torch
    rec = cli_case("hitdiff_percent")
    assert rec["args"] == ["-hitdiff", "80", "-maxcand", "3", "-lowest", "species", "-tophits", "-queryids"]
    golden = "".join(l + "\n" for l in rec["lines"] if l and not l.startswith("#")).encode()
    recs = read_fasta(os.path.join(GOLDEN, "cli_reads.fa"))
    reads = [s for _, s, _ in recs]
    dev = torch.device("cuda", 0)
    d = api.Database.open(os.path.join(GOLDEN, "toy32"), max_candidates=3)
    try:
        texts = api.mapping_texts(d.taxa(), d.taxon_table()[0], d.lineages(), lowest=4)
        for which, strings in texts.items():
            d.format_set_text(which, strings)
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
        capacity = len(golden) + 100
        out = torch.full((capacity,), FILL, dtype=torch.uint8, device=dev)
        line_off = torch.empty(n + 1 + api.FORMAT_SCRATCH, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        # the golden case's header: hit threshold 5, three candidates, ranks species .. domain, -hitdiff 80 = 80 %
        r = d.query_device(seq.data_ptr(), qi.data_ptr(), n, int(offs[-1]), max_win_ptr=dmw.data_ptr(), lowest=4)
        d.classify_device(r.cands, n, 3, out_ptr=assigned.data_ptr(), hitmin=5, hitdiff=80, lowest=4, highest=19)
        d.format_device(api.format_options(b"\t|\t", d.stride, d.w), r.cands, 3, assigned.data_ptr(), names.data_ptr(), name_off.data_ptr(), n,
                        flags=api.FORMAT_QUERY_IDS | api.FORMAT_TOPHITS, query_ids_ptr=ids.data_ptr(), out_ptr=out.data_ptr(), out_capacity=capacity,
                        line_off_ptr=line_off.data_ptr())
        d.synchronize()
        off = line_off[:n + 1].cpu().numpy()
        got = out.cpu().numpy()
        assert n == 399 and recs[-1][2] == 400 and int(off[-1]) == len(golden)
        assert got[:len(golden)].tobytes() == golden and (got[len(golden):] == FILL).all()
        assert [got[off[i]:off[i + 1]].tobytes() for i in (0, 398)] == [golden.split(b"\n")[0] + b"\n", golden.split(b"\n")[398] + b"\n"]
        assert d.format_stats() == [1, 399, 399, len(golden), 0]
    finally:
        d.close()
