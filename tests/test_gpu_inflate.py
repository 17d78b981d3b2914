"""GPU: mc_inflate_blocks (inflate.hip), the device form and MC_INFLATE_HOST, against zlib / gzip: every case of inflate_cases alone and
all in one call, block counts around the workgroup's four waves and beyond, rows permuted, every bad stream at three positions with the
status the model (inflate_ref) owes, out_capacity one short, the same call twice and on two streams, inflate -> parse on one stream, and
the host form in several staged pieces.  Every device output lies between 4 KiB guard zones, and what a call does not own must stay as
it was.  A good member that the device refuses FAILS here: there is no skip and no fall-back."""
import gzip
import os
import random
import zlib

import numpy as np
import pytest

import inflate_cases as cases
import inflate_ref as ref
from metacache_amd import api

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GUARD, FILL = 4096, 0xA5


@pytest.fixture(scope="module")
def db():
    d = api.Database.open(os.path.join(GOLDEN, "toy32"), max_candidates=2)
    yield d
    d.close()


def rows_of(data):
    rows, out_bytes, verdict, _ = ref.walk(data)
    assert verdict == ref.BGZF_OK
    return rows, out_bytes


def as_array(rows):
    return np.array(rows, dtype=api.bgzf_block_dtype)


def owed(data, rows, cap):
    """the status a call owes and, for an accepted one, the slices' bytes.  The oracle is gzip: a member it reads to out_len bytes is good;
    only for one it refuses is the model asked, for the reason (and the model must refuse it too)"""
    covered, bad, slices = 0, None, []
    for i, (in_off, out_off, in_len, out_len) in enumerate(rows):
        if out_off + out_len > cap:
            bad = bad or (ref.INFLATE_OVERFLOW, i, 0)
            continue
        covered = max(covered, out_off + out_len)
        member = data[in_off:in_off + in_len]
        try:
            plain = gzip.decompress(member)
            assert len(plain) == out_len
            slices.append((out_off, plain))
        except (OSError, EOFError, zlib.error):
            with pytest.raises(ref.Refused) as e:
                ref.inflate_member(member, out_len)
            bad = bad or (ref.INFLATE_CORRUPT, i, e.value.reason)
    return ([bad[0], bad[1], bad[2], covered] if bad else [ref.INFLATE_OK, 0, 0, covered]), slices


def image(data, rows, cap, fill, known=None):
    """what out[0, cap) must hold after an accepted call, and the status every call owes"""
    status, slices = known or owed(data, rows, cap)
    img = np.full(cap, fill, dtype=np.uint8)
    if status[0] == ref.INFLATE_OK:
        for out_off, plain in slices:
            img[out_off:out_off + len(plain)] = np.frombuffer(plain, dtype=np.uint8)
    return img, status


class OnDevice:
    """a range, its rows and out in device memory; out between two guard zones"""

    def __init__(self, data, rows, cap):
        import torch
        self.torch, dev = torch, torch.device("cuda", 0)
        self.n, self.cap, self.nrows = len(data), cap, len(rows)
        padded = np.zeros((len(data) + 15) // 16 * 16 + 16, dtype=np.uint8)
        padded[:len(data)] = np.frombuffer(data, dtype=np.uint8)
        self.bytes = torch.from_numpy(padded).to(dev)
        self.rows = torch.from_numpy(as_array(rows).view(np.uint8).copy() if len(rows) else np.zeros(24, dtype=np.uint8)).to(dev)
        self.out = torch.full((GUARD + (cap + 15) // 16 * 16 + GUARD,), FILL, dtype=torch.uint8, device=dev)
        self.status = torch.full((4,), -1, dtype=torch.int64, device=dev)
        assert self.bytes.data_ptr() % 16 == 0 and self.out.data_ptr() % 16 == 0 and self.rows.data_ptr() % 8 == 0
        torch.cuda.synchronize()

    def enqueue(self, db, stream=0):
        db.inflate_device(self.bytes.data_ptr(), self.n, self.rows.data_ptr(), self.nrows, self.out.data_ptr() + GUARD, self.cap, self.status.data_ptr(), stream=stream)
        return self

    def result(self):
        """-> (out[0, cap), status); everything outside out[0, cap) must be untouched"""
        self.torch.cuda.synchronize()
        raw = self.out.cpu().numpy()
        assert np.all(raw[:GUARD] == FILL), "bytes in front of out were written"
        assert np.all(raw[GUARD + self.cap:] == FILL), "bytes behind out_capacity were written"
        return raw[GUARD:GUARD + self.cap], [int(x) for x in self.status.cpu().numpy().view(np.uint64)]


def check_both_forms(db, data, rows, cap, what, host=True):
    known = owed(data, rows, cap)
    img, status = image(data, rows, cap, FILL, known)
    out, st = OnDevice(data, rows, cap).enqueue(db).result()
    assert st == status, f"{what} (device form): status {st}, owed {status}"
    if status[0] == ref.INFLATE_OK:
        assert np.array_equal(out, img), f"{what} (device form): bytes differ from zlib's, or a byte outside the slices was written"
    if host:
        himg, _ = image(data, rows, cap, 0, known)
        hout, hst = db.inflate_raw(data, as_array(rows), cap)
        assert [int(x) for x in hst] == status, f"{what} (host form): status {[int(x) for x in hst]}, owed {status}"
        if status[0] == ref.INFLATE_OK:
            assert np.array_equal(hout, himg), f"{what} (host form)"
    return status


# ---- the good cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.good_cases()))
def test_one_block(db, name):
    m, plain = cases.good_cases()[name]
    rows, out_bytes = rows_of(m)
    assert out_bytes == len(plain)
    assert check_both_forms(db, m, rows, len(plain), name) == [0, 0, 0, len(plain)]
    # the slice inside a larger out, not at its start and at an odd offset: nothing around it is written
    moved = [(0, 4099, len(m), len(plain))]
    assert check_both_forms(db, m, moved, 4099 + len(plain) + 4101, name + " inside a larger out") == [0, 0, 0, 4099 + len(plain)]
    assert db.inflate(m) == plain


def test_all_cases_in_one_call(db):
    good = cases.good_cases()
    data = b"".join(good[n][0] for n in sorted(good))
    rows, out_bytes = rows_of(data)
    assert check_both_forms(db, data, rows, out_bytes, "all cases") == [0, 0, 0, out_bytes]
    assert db.inflate(data) == gzip.decompress(data)
    before = db.inflate_stats()
    assert db.inflate(data) == gzip.decompress(data)
    after = db.inflate_stats()
    assert [a - b for a, b in zip(after, before)] == [1, len(data), out_bytes, 0]


@pytest.fixture(scope="module")
def pool():
    """300 small members of mixed kinds with their bytes, and a few whole ones among them"""
    rnd = random.Random(41)
    kinds = [(0, zlib.Z_DEFAULT_STRATEGY), (1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED),
             (6, zlib.Z_RLE), (6, zlib.Z_HUFFMAN_ONLY)]
    text = cases.fastq_text(300 * 2600, 29)
    members, at = [], 0
    good = cases.good_cases()
    whole = {7: "far_match", 63: "fibonacci_15bit", 64: "largest_expansion", 150: "eof", 299: "two_blocks_flush"}
    for i in range(300):
        if i in whole:
            members.append(good[whole[i]])
            continue
        n = rnd.randint(1, 2600)
        lv, st = kinds[i % len(kinds)]
        members.append((cases.bgzf_block(text[at:at + n], lv, st, flush_at=n // 2 if i % 11 == 0 else None), text[at:at + n]))
        at += n
    return members


@pytest.mark.parametrize("count", [1, 63, 64, 65, 300])
def test_block_counts_in_file_order_and_permuted(db, pool, count):
    data = b"".join(m for m, _ in pool[:count])
    plain = b"".join(p for _, p in pool[:count])
    rows, out_bytes = rows_of(data)
    assert len(rows) == count and out_bytes == len(plain)
    assert check_both_forms(db, data, rows, out_bytes, f"{count} blocks") == [0, 0, 0, out_bytes]
    shuffled = rows[:]
    random.Random(count).shuffle(shuffled)
    out, st = OnDevice(data, shuffled, out_bytes).enqueue(db).result()
    assert st == [0, 0, 0, out_bytes] and out.tobytes() == plain, f"{count} blocks, rows permuted"
    if count > 1 and shuffled != rows:
        with pytest.raises(api.McError):
            db.inflate_raw(data, as_array(shuffled), out_bytes)            # the host form takes rows in file order only


def test_host_form_in_several_pieces(db, pool):
    data = b"".join(m for m, _ in pool)
    plain = b"".join(p for _, p in pool)
    rows, out_bytes = rows_of(data)
    db.set_tuning("inflate_stage_bytes", len(data) // 5)
    try:
        db.timing(True)
        db.timing_reset()
        out, st = db.inflate_raw(data, as_array(rows), out_bytes)
        pieces = db.timing_get("inflate_blocks")[1]
        assert [int(x) for x in st] == [0, 0, 0, out_bytes] and out.tobytes() == plain
        assert 4 <= pieces <= 8, pieces
        # a bad block in the third piece: its number counts from the call's first row
        bad = cases.bad_cases()["wrong_crc"]
        k = 2 * len(rows) // 3
        data2 = b"".join(m for m, _ in pool[:k]) + bad + b"".join(m for m, _ in pool[k:])
        rows2 = ref.walk(data2)[0]
        _, st = db.inflate_raw(data2, as_array(rows2), ref.walk(data2)[1])
        assert [int(x) for x in st][:3] == [ref.INFLATE_CORRUPT, k, ref.R_CRC]
    finally:
        db.timing(False)
        db.set_tuning("inflate_stage_bytes", 0)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def neighbours():
    good = cases.good_cases()
    return [good[n] for n in ("short_text", "one_byte", "bc_behind_another_subfield", "eof", "short_text", "one_byte")]


@pytest.mark.parametrize("name", sorted(cases.bad_cases()))
def test_bad_stream_at_three_positions(db, name):
    bad = cases.bad_cases()[name]
    good = neighbours()
    for pos in (0, len(good) // 2, len(good)):
        members = [m for m, _ in good[:pos]] + [bad] + [m for m, _ in good[pos:]]
        data = b"".join(members)
        rows, out_bytes = ref.walk(data)[:2]
        st = check_both_forms(db, data, rows, out_bytes, f"{name} at {pos}")
        assert st[0] == ref.INFLATE_CORRUPT and st[1] == pos and st[2] != 0
        with pytest.raises(api.McError) as e:
            db.inflate(data)
        assert (e.value.verdict, e.value.block, e.value.reason) == tuple(st[:3])


def test_two_bad_blocks_report_the_lower(db):
    bad, good = cases.bad_cases(), neighbours()
    members = [good[0][0], good[1][0], bad["wrong_crc"], good[2][0], bad["block_type_3"], good[3][0]]
    data = b"".join(members)
    rows, out_bytes = ref.walk(data)[:2]
    assert check_both_forms(db, data, rows, out_bytes, "two bad blocks")[:3] == [ref.INFLATE_CORRUPT, 2, ref.R_CRC]
    members[2], members[4] = members[4], members[2]
    data = b"".join(members)
    rows, out_bytes = ref.walk(data)[:2]
    assert check_both_forms(db, data, rows, out_bytes, "two bad blocks, swapped")[:3] == [ref.INFLATE_CORRUPT, 2, ref.R_BTYPE]
    # the rows the other way round: the lowest ROW decides
    out, st = OnDevice(data, rows[::-1], out_bytes).enqueue(db).result()
    assert st[:3] == [ref.INFLATE_CORRUPT, 1, ref.R_CRC]


def test_capacity_one_short_is_overflow(db):
    good = neighbours()
    data = b"".join(m for m, _ in good)
    rows, out_bytes = rows_of(data)
    last = max(i for i, r in enumerate(rows) if r[3] > 0)
    st = check_both_forms(db, data, rows, out_bytes - 1, "capacity one short")
    assert st[:3] == [ref.INFLATE_OVERFLOW, last, 0]
    assert check_both_forms(db, data, rows, 0, "no capacity")[:3] == [ref.INFLATE_OVERFLOW, 0, 0]
    assert check_both_forms(db, b"", [], 0, "no rows") == [0, 0, 0, 0]


def test_same_call_twice_and_on_two_streams(db, pool):
    import torch
    data = b"".join(m for m, _ in pool[:130])
    plain = b"".join(p for _, p in pool[:130])
    rows, out_bytes = rows_of(data)
    streams = [torch.cuda.Stream(device=torch.device("cuda", 0)) for _ in range(2)]
    calls = [OnDevice(data, rows, out_bytes) for _ in range(4)]
    for k, c in enumerate(calls):
        c.enqueue(db, stream=streams[k % 2].cuda_stream)
    for s in streams:
        s.synchronize()
    for c in calls:
        out, st = c.result()
        assert st == [0, 0, 0, out_bytes] and out.tobytes() == plain
    again = calls[0].enqueue(db).result()
    assert again[1] == [0, 0, 0, out_bytes] and again[0].tobytes() == plain


# ---- inflate -> parse on one stream, nothing waited for in between --------------------------------------------------------------------------
def test_chain_into_the_device_parse(db):
    import torch
    with open(os.path.join(GOLDEN, "cli_pairs.fq"), "rb") as f:
        plain = f.read()
    data = cases.bgzf_file(plain, payload=3000)
    rows, out_bytes = rows_of(data)
    assert out_bytes == len(plain) and len(rows) > 4
    want = db.parse_records(plain, pairs=True)
    ws = [int(x) for x in want["status"]]
    assert ws[4] == api.PARSE_OK
    recs, queries, seq_need, name_need = ws[:4]
    dev = torch.device("cuda", 0)
    d = OnDevice(data, rows, out_bytes)
    z = lambda n, dt: torch.zeros(max(n, 1), dtype=dt, device=dev)
    hdr, qinfo, seq, names = z(2 * recs, torch.int32), z(4 * recs, torch.int32), z(seq_need + 16, torch.uint8), z(name_need + 16, torch.uint8)
    name_off, max_win, status = z(recs + 1, torch.int64), z(recs, torch.int32), z(8, torch.int64)
    wsb = api.parse_scratch_bytes(out_bytes)
    work = z(wsb, torch.uint8)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=dev)
    d.enqueue(db, stream=s.cuda_stream)
    db.parse_device(d.out.data_ptr() + GUARD, out_bytes, hdr_ptr=hdr.data_ptr(), qinfo_ptr=qinfo.data_ptr(), seq_ptr=seq.data_ptr(), seq_capacity=seq_need,
                    names_ptr=names.data_ptr(), names_capacity=name_need, name_off_ptr=name_off.data_ptr(), max_win_ptr=max_win.data_ptr(), status_ptr=status.data_ptr(),
                    max_records=recs, workspace_ptr=work.data_ptr(), workspace_bytes=wsb, pairs=True, stream=s.cuda_stream)
    s.synchronize()
    out, st = d.result()
    assert st == [0, 0, 0, out_bytes] and out.tobytes() == plain
    host = lambda t, dt: t.cpu().numpy().view(dt)
    assert [int(x) for x in host(status, np.uint64)] == ws
    assert np.array_equal(host(hdr, np.uint32)[:2 * recs].reshape(recs, 2), want["hdr"])
    assert np.array_equal(host(qinfo, np.uint32)[:4 * queries].reshape(queries, 4), want["qinfo"])
    assert host(seq, np.uint8)[:seq_need].tobytes() == want["seq"] and host(names, np.uint8)[:name_need].tobytes() == want["names"]
    assert np.array_equal(host(name_off, np.uint64)[:queries + 1], want["name_off"]) and np.array_equal(host(max_win, np.uint32)[:queries], want["max_win"])
