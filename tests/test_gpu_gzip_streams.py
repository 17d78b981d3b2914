"""GPU: mc_inflate_streams (inflate_streams.hip), the device form and MC_INFLATE_HOST, against the model of the stream rule (gzip_ref),
byte for byte: every row of gzip_cases alone, row counts around a wave's 64 and beyond, rows permuted, in_off at every residue mod 16,
every bad row among good ones with each row's own verdict, out_cap larger than produced, two streams at once, inflate -> parse_targets ->
parse_headers on one stream, and the host form in several staged pieces.  Every device output lies between 4 KiB guard zones AND has a
4 KiB guard zone between neighbouring rows' slices; what a row does not own must stay as it was.  A good row that the device refuses
FAILS here: there is no skip and no fall-back."""
import os
import random
import zlib

import numpy as np
import pytest

import gzip_cases as cases
import gzip_ref as ref
from metacache_amd import api

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GUARD, FILL = 4096, 0xA5
KNOWN = {}          # (row bytes, out_cap) -> the model's answer, computed once per module


@pytest.fixture(scope="module")
def db():
    d = api.Database.open(os.path.join(GOLDEN, "toy32"), max_candidates=2)
    yield d
    d.close()


def know_good(row, plain, caps):
    """the model's answer for a good row, computed once (at the smallest room) and entered for every room that holds it"""
    key = (row, len(plain))
    if key not in KNOWN:
        KNOWN[key] = ref.inflate_row(row, len(plain))
        assert KNOWN[key][0] == plain
    for cap in caps:
        assert cap >= len(plain)
        KNOWN[(row, cap)] = KNOWN[key]


def layout(items, gap=GUARD, first_residue=0):
    """items [(row bytes, out_cap)] -> (data, rows [(in_off, in_len, out_off, out_cap)], out_capacity): row i's bytes begin at residue
    (first_residue + i) mod 16, the slices lie `gap` bytes apart"""
    parts, rows, at, out_at = [], [], 0, 0
    for i, (row, cap) in enumerate(items):
        pad = ((first_residue + i) - at) % 16
        parts.append(bytes([0x1f] * pad))            # (what lies between rows looks like the start of a member)
        at += pad
        rows.append((at, len(row), out_at, cap))
        parts.append(row)
        at += len(row)
        out_at += cap + gap
    return b"".join(parts), rows, max(out_at - gap, 0)


def as_array(rows):
    return np.array(rows, dtype=api.gzip_stream_dtype) if len(rows) else np.zeros(0, dtype=api.gzip_stream_dtype)


class OnDevice:
    """a range, its rows, out, results and status in device memory; out between two guard zones"""

    def __init__(self, data, rows, cap):
        import torch
        self.torch, dev = torch, torch.device("cuda", 0)
        self.n, self.cap, self.nrows = len(data), cap, len(rows)
        padded = np.zeros((len(data) + 15) // 16 * 16 + 16, dtype=np.uint8)
        padded[:len(data)] = np.frombuffer(data, dtype=np.uint8)
        self.bytes = torch.from_numpy(padded).to(dev)
        self.rows = torch.from_numpy(as_array(rows).view(np.uint8).copy() if len(rows) else np.zeros(32, dtype=np.uint8)).to(dev)
        self.out = torch.full((GUARD + (cap + 15) // 16 * 16 + GUARD,), FILL, dtype=torch.uint8, device=dev)
        self.results = torch.full((16 * max(len(rows), 1) + GUARD,), FILL, dtype=torch.uint8, device=dev)
        self.status = torch.full((4,), -1, dtype=torch.int64, device=dev)
        assert self.bytes.data_ptr() % 16 == 0 and self.out.data_ptr() % 16 == 0 and self.rows.data_ptr() % 8 == 0 and self.results.data_ptr() % 8 == 0
        torch.cuda.synchronize()

    def enqueue(self, db, stream=0):
        db.inflate_streams_device(self.bytes.data_ptr(), self.n, self.rows.data_ptr(), self.nrows, self.out.data_ptr() + GUARD, self.cap, self.results.data_ptr(),
                                  self.status.data_ptr(), stream=stream)
        return self

    def result(self):
        """-> (out[0, cap), results, status); everything outside out[0, cap) and behind the results must be untouched"""
        self.torch.cuda.synchronize()
        raw = self.out.cpu().numpy()
        assert np.all(raw[:GUARD] == FILL), "bytes in front of out were written"
        assert np.all(raw[GUARD + self.cap:] == FILL), "bytes behind out_capacity were written"
        res = self.results.cpu().numpy()
        assert np.all(res[16 * self.nrows:] == FILL), "bytes behind the results were written"
        return raw[GUARD:GUARD + self.cap], res[:16 * self.nrows].view(api.gzip_result_dtype), [int(x) for x in self.status.cpu().numpy().view(np.uint64)]


def assert_owed(out, results, status, owed, rows, fill, what):
    """status and results are the model's; an accepted row's slice holds the model's bytes and `fill` behind them; outside the slices of
    the refused rows (which may hold anything) every byte is `fill`: the guard zones between the rows are intact"""
    want_status, want_results, good = owed
    assert status == want_status, f"{what}: status {status}, owed {want_status}"
    got = [(int(r["produced"]), int(r["members"]), int(r["reason"])) for r in results]
    assert got == want_results, f"{what}: results differ at rows {[i for i, (g, w) in enumerate(zip(got, want_results)) if g != w][:8]}"
    img = np.full(len(out), fill, dtype=np.uint8)
    own = np.zeros(len(out), dtype=bool)
    for i, (_, _, out_off, out_cap) in enumerate(rows):
        if i in good:
            img[out_off:out_off + len(good[i])] = np.frombuffer(good[i], dtype=np.uint8)
        elif out_off + out_cap <= len(out):
            own[out_off:out_off + out_cap] = True
    same = (out == img) | own
    assert same.all(), f"{what}: byte {int(np.argmin(same))} of out differs from the model's, or lies outside every slice and was written"


def check_both_forms(db, data, rows, cap, what, host=True, device=True):
    owed = ref.expected(data, rows, cap, KNOWN)
    if device:
        out, results, st = OnDevice(data, rows, cap).enqueue(db).result()
        assert_owed(out, results, st, owed, rows, FILL, what + " (device form)")
    if host:
        hout, hres, hst = db.inflate_streams_raw(data, as_array(rows), cap)
        assert_owed(hout, hres, [int(x) for x in hst], owed, rows, 0, what + " (host form)")
    return owed[0]


# ---- the good rows ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.good_cases()))
def test_one_row(db, name):
    row, plain = cases.good_cases()[name]
    know_good(row, plain, [len(plain)])
    data, rows, cap = layout([(row, len(plain))], first_residue=len(name) % 16)
    assert check_both_forms(db, data, rows, cap, name) == [0, 0, 0, 1]
    # the slice inside a larger out, not at its start and at an odd offset: nothing around it is written
    moved = [(rows[0][0], rows[0][1], 4099, len(plain))]
    assert check_both_forms(db, data, moved, 4099 + len(plain) + 4101, name + " inside a larger out", host=len(plain) < 300000) == [0, 0, 0, 1]


def test_the_python_face_and_the_stats(db):
    good = cases.good_cases()
    names = ["fname", "chain_of_2", "empty_file", "fextra_fname_fcomment"]
    files = [good[n][0] for n in names]
    before = db.inflate_streams_stats()
    plain, results = db.inflate_streams(files, out_caps=[len(good[n][1]) for n in names])
    assert plain == [good[n][1] for n in names] and [int(r["members"]) for r in results] == [1, 2, 1, 1]
    after = db.inflate_streams_stats()
    assert [a - b for a, b in zip(after, before)] == [1, sum((len(f) + 15) // 16 * 16 for f in files), sum(len(p) for p in plain), 0]
    # rooms from the trailing ISIZE: right for single members, too small for the chain, which says so and leaves the others as they are
    plain, results = db.inflate_streams(files)
    assert plain == [good["fname"][1], None, b"", good["fextra_fname_fcomment"][1]] and int(results[1]["reason"]) == ref.R_OVER
    assert db.inflate_streams_stats()[3] - after[3] == 1


@pytest.fixture(scope="module")
def pool():
    """257 small rows of mixed kinds with their bytes -- levels, strategies, header fields, chains -- and a few whole cases among them"""
    rnd = random.Random(41)
    kinds = [(0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED),
             (6, zlib.Z_RLE), (6, zlib.Z_HUFFMAN_ONLY)]
    text = cases.fasta_text(257 * 2600, 29)
    good = cases.good_cases()
    whole = {7: "match_3_at_32768_across_65536", 63: "chain_of_3", 64: "chain_empty_first", 150: "empty_file", 256: "fname_zero_in_the_next_round"}
    rows, at = [], 0
    for i in range(257):
        if i in whole:
            rows.append(good[whole[i]])
            continue
        n = rnd.randint(1, 2600)
        lv, st = kinds[i % len(kinds)]
        plain = text[at:at + n]
        at += n
        m = cases.member(cases.raw_deflate(plain, lv, st, flush_every=n // 3 + 1 if i % 11 == 0 else None), plain, name=b"file%d.fa" % i if i % 3 == 0 else None,
                         extra=b"xy" if i % 5 == 0 else None)
        if i % 13 == 0:
            m += cases.gz(plain[:n // 2])
            plain += plain[:n // 2]
        rows.append((m, plain))
    for row, plain in rows:
        know_good(row, plain, [len(plain), len(plain) + 1000])
    return rows


@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_row_counts_in_order_and_permuted(db, pool, count):
    data, rows, cap = layout([(r, len(p)) for r, p in pool[:count]], first_residue=count)
    if count >= 16:
        assert {r[0] % 16 for r in rows} == set(range(16))
    assert check_both_forms(db, data, rows, cap, f"{count} rows") == [0, 0, 0, count]
    shuffled = rows[:]
    random.Random(count).shuffle(shuffled)
    assert check_both_forms(db, data, shuffled, cap, f"{count} rows, permuted") == [0, 0, 0, count]


def test_out_cap_larger_than_produced(db, pool):
    data, rows, cap = layout([(r, len(p) + 1000) for r, p in pool[100:140]], first_residue=3)
    owed = ref.expected(data, rows, cap, KNOWN)
    assert [r[0] for r in owed[1]] == [len(p) for _, p in pool[100:140]]            # produced is the bytes, not the room
    assert check_both_forms(db, data, rows, cap, "rooms larger than the bytes") == [0, 0, 0, 40]


# ---- a row's verdict is its own ---------------------------------------------------------------------------------------------------------
def test_every_bad_row_among_good_rows(db, pool):
    bad = cases.bad_cases()
    items, names = [], []
    for k, name in enumerate(sorted(bad)):
        items.append((pool[k][0], len(pool[k][1])))
        names.append(None)
        items.append((bad[name][0], bad[name][1]))
        names.append(name)
    items.append((pool[40][0], len(pool[40][1])))
    names.append(None)
    data, rows, cap = layout(items, first_residue=5)
    rows.append((rows[0][0], rows[0][1], cap + 1, 16))              # a slice outside out_capacity: R_OVER, writes nothing
    names.append("slice outside out_capacity")
    owed = ref.expected(data, rows, cap, KNOWN)
    for i, name in enumerate(names):
        if name is None:
            assert owed[1][i][2] == 0 and i in owed[2]
        elif name in bad:
            assert owed[1][i][2] == bad[name][2], name
    assert owed[1][-1] == (0, 0, ref.R_OVER)
    first_bad = sorted(bad)[0]
    assert owed[0] == [ref.INFLATE_OVERFLOW if bad[first_bad][2] == ref.R_OVER else ref.INFLATE_CORRUPT, 1, bad[first_bad][2], len(bad) + 1]
    assert check_both_forms(db, data, rows, cap, "bad rows among good ones", host=False) == owed[0]
    # the host form refuses a row below 18 bytes as an argument; the others as the device form does
    keep = [i for i, n in enumerate(names) if n not in cases.HOST_ARGUMENT_ERRORS]
    hrows = [rows[i] for i in keep]
    assert check_both_forms(db, data, hrows, cap, "bad rows among good ones", device=False)[3] == len(bad) + 1
    with pytest.raises(api.McError):
        db.inflate_streams_raw(data, as_array(rows), cap)
    # the rows the other way round: the lowest ROW decides
    back = rows[::-1]
    st = check_both_forms(db, data, back, cap, "the same rows from the last to the first", host=False)
    assert st[:3] == [ref.INFLATE_OVERFLOW, 0, ref.R_OVER]
    # each bad row alone: the call's verdict is the row's
    for name in ("second_member_reaches_into_the_first", "trailing_zeros", "fhcrc", "out_cap_one_short"):
        d1, r1, c1 = layout([(bad[name][0], bad[name][1])], first_residue=7)
        st = check_both_forms(db, d1, r1, c1, name)
        assert st == [ref.INFLATE_OVERFLOW if bad[name][2] == ref.R_OVER else ref.INFLATE_CORRUPT, 0, bad[name][2], 0]
    assert check_both_forms(db, b"", [], 0, "no rows") == [0, 0, 0, 0]


def test_same_call_on_two_streams_at_once(db, pool):
    import torch
    data, rows, cap = layout([(r, len(p)) for r, p in pool[:130]])
    owed = ref.expected(data, rows, cap, KNOWN)
    streams = [torch.cuda.Stream(device=torch.device("cuda", 0)) for _ in range(2)]
    calls = [OnDevice(data, rows, cap) for _ in range(4)]
    for k, c in enumerate(calls):
        c.enqueue(db, stream=streams[k % 2].cuda_stream)
    for s in streams:
        s.synchronize()
    for k, c in enumerate(calls):
        out, results, st = c.result()
        assert_owed(out, results, st, owed, rows, FILL, f"call {k}")
    out, results, st = calls[0].enqueue(db).result()
    assert_owed(out, results, st, owed, rows, FILL, "the first call again")


# ---- inflate -> parse_targets -> parse_headers on one stream, nothing waited for in between: the path of `mcq build` -----------------------
def test_chain_into_the_target_parse(db):
    import torch
    files = [cases.fasta_text(n, seed) for n, seed in ((5000, 51), (70000, 52), (1200, 53), (33333, 54))]
    gz = [cases.gz(f, name=b"g%d.fna" % i if i % 2 else None) for i, f in enumerate(files)]
    plain = b"".join(files)
    off = np.cumsum([0] + [len(f) for f in files]).astype(np.uint64)
    want = db.parse_targets(plain, off)
    ws = [int(x) for x in want["status"]]
    assert ws[4] == api.PARSE_OK
    recs, seq_need = ws[0], ws[2]
    want_h = db.parse_headers(plain, want["hdr"], want["status"])
    assert int(want_h["status"][2]) == api.PARSE_OK
    # the rows: compressed bytes at any residue, the slices touching: out is the piece
    parts, rows, at = [], [], 0
    for i, g in enumerate(gz):
        pad = (5 * i + 3 - at) % 16
        parts.append(bytes(pad))
        at += pad
        rows.append((at, len(g), int(off[i]), len(files[i])))
        parts.append(g)
        at += len(g)
    d = OnDevice(b"".join(parts), rows, len(plain))
    dev = torch.device("cuda", 0)
    z = lambda n, dt: torch.zeros(max(n, 1), dtype=dt, device=dev)
    file_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
    hdr, targets, seq, status = z(2 * recs, torch.int32), z(recs * api.parse_target_dtype.itemsize, torch.uint8), z(seq_need + 16, torch.uint8), z(8, torch.int64)
    wsb = api.parse_targets_scratch_bytes(len(plain), len(files), recs)
    work = z(wsb, torch.uint8)
    hout, hoff, hst = z(len(plain), torch.uint8), z(recs + 1, torch.int64), z(4, torch.int64)
    hwsb = api.parse_headers_scratch_bytes(recs)
    hwork = z(hwsb, torch.uint8)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=dev)
    piece = d.out.data_ptr() + GUARD
    d.enqueue(db, stream=s.cuda_stream)
    db.parse_targets_device(piece, len(plain), file_off.data_ptr(), len(files), hdr_ptr=hdr.data_ptr(), targets_ptr=targets.data_ptr(), seq_ptr=seq.data_ptr(),
                            seq_capacity=seq_need, status_ptr=status.data_ptr(), max_records=recs, workspace_ptr=work.data_ptr(), workspace_bytes=wsb, stream=s.cuda_stream)
    db.parse_headers_device(piece, len(plain), hdr_ptr=hdr.data_ptr(), parse_status_ptr=status.data_ptr(), max_records=recs, out_ptr=hout.data_ptr(),
                            out_capacity=len(plain), out_off_ptr=hoff.data_ptr(), status_ptr=hst.data_ptr(), workspace_ptr=hwork.data_ptr(), workspace_bytes=hwsb,
                            stream=s.cuda_stream)
    s.synchronize()
    out, results, st = d.result()
    assert st == [0, 0, 0, len(files)] and out.tobytes() == plain
    assert [(int(r["produced"]), int(r["reason"])) for r in results] == [(len(f), 0) for f in files]
    host = lambda t, dt: t.cpu().numpy().view(dt)
    assert [int(x) for x in host(status, np.uint64)] == ws
    assert np.array_equal(host(hdr, np.uint32)[:2 * recs].reshape(recs, 2), want["hdr"])
    assert host(targets, np.uint8).tobytes() == want["targets"].tobytes() and host(seq, np.uint8)[:seq_need].tobytes() == want["seq"]
    assert [int(x) for x in host(hst, np.uint64)] == [int(x) for x in want_h["status"]]
    n = int(want_h["status"][1])
    assert host(hout, np.uint8)[:n].tobytes() == want_h["out"] and np.array_equal(host(hoff, np.uint64)[:recs + 1], want_h["out_off"])


def test_host_form_in_several_pieces(db, pool):
    data, rows, cap = layout([(r, len(p)) for r, p in pool], gap=0)
    db.set_tuning("inflate_stage_bytes", len(data) // 4)
    try:
        db.timing(True)
        db.timing_reset()
        owed = ref.expected(data, rows, cap, KNOWN)
        hout, hres, hst = db.inflate_streams_raw(data, as_array(rows), cap)
        pieces = db.timing_get("inflate_streams")[1]
        assert_owed(hout, hres, [int(x) for x in hst], owed, rows, 0, "in pieces")
        assert owed[0] == [0, 0, 0, len(rows)] and hout.tobytes() == b"".join(p for _, p in pool)
        assert 3 <= pieces <= 16, pieces
        # bad rows in the second and in the last piece: their numbers count from the call's first row, the rest is as it was
        bad = cases.bad_cases()
        items = [(r, len(p)) for r, p in pool]
        k1, k2 = len(items) // 2, len(items) - 3
        items[k1] = bad["wrong_crc_in_the_first_of_two"][:2]
        items[k2] = bad["trailing_garbage"][:2]
        data2, rows2, cap2 = layout(items, gap=0)
        owed2 = ref.expected(data2, rows2, cap2, KNOWN)
        assert owed2[0] == [ref.INFLATE_CORRUPT, k1, ref.R_CRC, len(items) - 2]
        hout, hres, hst = db.inflate_streams_raw(data2, as_array(rows2), cap2)
        assert_owed(hout, hres, [int(x) for x in hst], owed2, rows2, 0, "in pieces, two bad rows")
    finally:
        db.timing(False)
        db.set_tuning("inflate_stage_bytes", 0)
