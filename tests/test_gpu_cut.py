"""GPU: mc_parse_cut and mc_parse_headers (parse_cut.hip), the device forms and MC_PARSE_HOST, against the cut rule in plain Python
(cut_ref), and the slot that takes device bytes (mc_batch_add_device_bytes, mc_batch_headers) against the slot that takes host bytes.

  * every case of cut_cases (the parse cases built around the tile T = api.parse_tile(), the golden files, the ranges whose END is the
    point), closed and open, every status word and every cut, with guard zones around cuts and status;
  * shapes at which the kernels can go wrong: record i * R starting at byte T - 1, T, T + 1; consumed at T - 1, T, T + 1; an offence in
    the tile that holds consumed, on either side of it; a last tile of one byte; 257 tiles (a second trip of the one-block scan); one record
    of 2.5 T; R = 1, R = whole, R > whole; bytes at 1, 15 and 17 from a 16-byte border; pairs with an odd count;
  * a range of 2^31 bytes (the largest the call takes), at a 16-byte border and one byte behind it;
  * a capacity one short (OVERFLOW, arrays untouched), two streams at once, a batch cut again with R / 2 (a refinement), inflate -> cut on
    one stream;
  * mc_parse_headers at 0, 1, 255, 256, 257 and 65 537 records, a header across a tile border, an empty header, a capacity one short, a
    parse that refused;
  * query_device_bytes on each batch of a cut file against query_file_bytes on the same bytes, from unaligned addresses."""
import os

import numpy as np
import pytest

import cut_cases
import cut_ref
import inflate_cases
import inflate_ref
import parse_cases
import parse_ref
from parse_cases import dna, fasta_record, fastq_record, pad_to
from metacache_amd import api

pytestmark = pytest.mark.gpu
GOLDEN = parse_cases.GOLDEN
GUARD, FILL = 64, 0xA5
FILL64 = int(np.array([FILL] * 8, dtype=np.uint8).view(np.int64)[0])


@pytest.fixture(scope="module")
def db():
    d = api.Database.open(os.path.join(GOLDEN, "toy32"), max_candidates=3)
    yield d
    d.close()


CASES = None


def cases():
    global CASES
    if CASES is None:
        CASES = cut_cases.all_cases(api.parse_tile())
    return CASES


CASE_NAMES = sorted(cut_cases.all_cases(4096))                     # (the names do not depend on the tile)


class OnDevice:
    """a range at `shift` bytes behind a 16-byte border, cuts and status between guard zones, the workspace with a guard behind it"""

    def __init__(self, data, capacity, shift=0):
        import torch
        self.torch, dev = torch, torch.device("cuda", 0)
        self.n, self.capacity, self.shift = len(data), capacity, shift
        room = np.full(shift + len(data) + 48, ord("\n"), dtype=np.uint8)    # ('\n' around the range: a kernel that reads outside it sees line starts)
        room[shift:shift + len(data)] = np.frombuffer(data, dtype=np.uint8)
        self.bytes = torch.from_numpy(room).to(dev)
        self.cuts = torch.full((GUARD + capacity + GUARD,), FILL64, dtype=torch.int64, device=dev)
        self.status = torch.full((GUARD + 8 + GUARD,), FILL64, dtype=torch.int64, device=dev)
        self.ws_bytes = api.parse_cut_scratch_bytes(self.n)
        self.ws = torch.full((self.ws_bytes + GUARD,), FILL, dtype=torch.uint8, device=dev)
        assert self.bytes.data_ptr() % 16 == 0 and self.ws.data_ptr() % 16 == 0
        torch.cuda.synchronize()

    def ptr(self):
        return self.bytes.data_ptr() + self.shift

    def enqueue(self, db, R, pairs=False, open_end=False, stream=0):
        db.parse_cut_device(self.ptr(), self.n, R, cuts_ptr=self.cuts.data_ptr() + 8 * GUARD, capacity=self.capacity, status_ptr=self.status.data_ptr() + 8 * GUARD,
                            workspace_ptr=self.ws.data_ptr(), workspace_bytes=self.ws_bytes, pairs=pairs, open=open_end, stream=stream)
        return self

    def result(self):
        """-> (status [8], cuts [capacity] as they lie in memory); the guard zones must be untouched"""
        self.torch.cuda.synchronize()
        cuts, status, ws = (t.cpu().numpy() for t in (self.cuts, self.status, self.ws))
        for name, a, used in (("cuts", cuts, self.capacity), ("status", status, 8)):
            assert np.all(a[:GUARD] == FILL64) and np.all(a[GUARD + used:] == FILL64), f"{name}: words outside the array were written"
        assert np.all(ws[self.ws_bytes:] == FILL), "bytes behind the workspace were written"
        return [int(x) for x in status[GUARD:GUARD + 8].view(np.uint64)], cuts[GUARD:GUARD + self.capacity].view(np.uint64)


def check(db, data, R, pairs=False, open_end=False, shift=0, host=True, what=""):
    """the device form (and the host form) against the model -> the model's cut"""
    want = cut_ref.cut(data, R, pairs, open_end)
    what = f"{what} R={R} pairs={pairs} open={open_end} shift={shift}"
    nb = -(-want.whole // R)
    st, cuts = OnDevice(data, nb + 1, shift).enqueue(db, R, pairs, open_end).result()
    forms = [("device", st, cuts)]
    if host and shift == 0:
        h = db.parse_cut(data, R, pairs=pairs, open=open_end, capacity=nb + 1)
        forms.append(("host", [int(x) for x in h["status"]], h["raw"]))
    for form, st, cuts in forms:
        if want.verdict != parse_ref.OK:
            assert st[4:6] == [want.verdict, want.offence], f"{what} ({form}): status {st}, the model refuses at {want.offence}"
            assert np.all(cuts.view(np.int64) == (FILL64 if form == "device" else 0)), f"{what} ({form}): cuts written with a refusing verdict"
            continue
        assert st == [want.whole, nb, want.consumed, want.seen, parse_ref.OK, 0, want.longest, want.half], f"{what} ({form}): status {st}, model {cut_ref.status_of(want)}"
        assert [int(x) for x in cuts[:nb + 1]] == want.cuts, f"{what} ({form})"
    return want


@pytest.mark.parametrize("name", CASE_NAMES)
def test_cases_against_the_model(db, name):
    data, pairs = cases()[name]
    for open_end in (False, True):
        whole = cut_ref.cut(data, 2, pairs, open_end).whole
        last = max(whole, 1) + (max(whole, 1) & 1 if pairs else 0)
        small = [23 + pairs] if len(data) > 1 << 18 else [1 + pairs, 23 + pairs]     # (the large files: the model takes its time)
        for R in small + [last, last + 1 + pairs]:
            check(db, data, R, pairs, open_end, what=name)


# ---- shapes built around the tile -------------------------------------------------------------------------------------------------------
def records_to(target, rng, fq):
    return pad_to(0, target, rng, fq)


@pytest.mark.parametrize("fq", [False, True])
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_selected_record_and_consumed_at_the_tile_border(db, fq, delta):
    T = api.parse_tile()
    rng = np.random.default_rng(21 + delta)
    rec = fastq_record if fq else fasta_record
    head = records_to(T + delta, rng, fq)
    k = len(parse_ref.parse(head).records)                          # the record that starts at T + delta has number k
    data = head + rec(b"at the border", dna(rng, 70)) + rec(b"after it", dna(rng, 33)) + rec(b"last", dna(rng, 20))
    assert data[T + delta:T + delta + 1] in (b">", b"@")
    for R in {1, k, max(k // 2, 1), k + 1, k + 3}:                  # R = k: cuts[1] is the record at the border
        want = check(db, data, R, what=f"record {k} at T{delta:+d}")
        if R == k:
            assert want.cuts[1] == T + delta
    # consumed at T + delta: the open range ends inside the record that starts there
    piece = head + rec(b"cut short", dna(rng, 70))[:40]
    want = check(db, piece, 2, open_end=True, what=f"consumed at T{delta:+d}")
    assert want.consumed == T + delta and want.whole == k
    # ... with an offence in the tile that holds consumed, in front of it and behind it
    bad = (b"@b\n+CGT\n+\nIIII\n" if fq else b">b\nAC\n+\nGT\n")
    front = records_to(T + delta - len(bad), rng, fq) + bad + rec(b"cut short", dna(rng, 70))[:40]
    want = check(db, front, 2, open_end=True, what=f"offence in front of consumed at T{delta:+d}")
    assert want.verdict == parse_ref.IRREGULAR and T + delta - len(bad) < want.offence < T + delta
    behind = head + bad[:-2]
    want = check(db, behind, 2, open_end=True, what=f"offence behind consumed at T{delta:+d}")
    assert want.verdict == parse_ref.OK and want.consumed == T + delta
    assert check(db, behind, 2, what="the same range, closed").verdict == parse_ref.IRREGULAR


def test_last_tile_of_one_byte_and_a_long_record(db):
    T = api.parse_tile()
    rng = np.random.default_rng(22)
    for fq in (False, True):
        data = records_to(T + 1, rng, fq)
        assert len(data) == T + 1
        marker = records_to(T, rng, fq) + (b"@" if fq else b">")        # ... and one whose only byte starts a record
        for open_end in (False, True):
            check(db, data, 2, open_end=open_end, what="a last tile of one byte")
            check(db, marker, 2, open_end=open_end, what="a last tile that is a marker")
    one = fasta_record(b"long one", dna(rng, 5 * T // 2), 60)
    check(db, one, 1, what="one record of 2.5 T")
    assert check(db, one, 1, open_end=True, what="one record of 2.5 T, open").consumed == 0
    three = fasta_record(b"before", dna(rng, 77), 60) + one + fasta_record(b"behind", dna(rng, 61), 60)
    for R in (1, 2, 3, 4):
        check(db, three, R, what="a record of 2.5 T between two")
        check(db, three, R, open_end=True, what="a record of 2.5 T between two")
    assert check(db, b">", 1).cuts == [0, 1] and check(db, b">", 1, open_end=True).cuts == [0]
    assert check(db, b"@", 1).verdict == parse_ref.IRREGULAR


def test_257_tiles(db):
    T = api.parse_tile()
    data, _ = cases()["many_tiles_fq"]
    assert len(data) > 257 * T
    data = data[:256 * T + 100]                                      # 257 tiles; the range ends inside a record
    want = check(db, data, 1, open_end=True, host=False, what="257 tiles")
    assert want.consumed > 256 * T - 400
    check(db, data, want.whole, open_end=True, host=False, what="257 tiles")
    check(db, data, 7, open_end=True, what="257 tiles")
    fa, _ = cases()["many_tiles_fa"]
    fa = fa[:256 * T + 1]
    check(db, fa, 1000, open_end=True, host=False, what="257 tiles, the last of one byte")
    check(db, fa, 1000, host=False, what="257 tiles, the last of one byte")


@pytest.mark.parametrize("shift", [1, 15, 17])
def test_bytes_at_any_address(db, shift):
    T = api.parse_tile()
    rng = np.random.default_rng(shift)
    for fq in (False, True):
        data = records_to(T - shift, rng, fq) + records_to(T + 40, rng, fq) + (fastq_record if fq else fasta_record)(b"end", dna(rng, 30))
        for open_end in (False, True):
            for R in (1, 5):
                check(db, data, R, open_end=open_end, shift=shift, what=f"fq={fq}")
        check(db, data[:37], 1, open_end=True, shift=shift, what="a range inside one load")
    check(db, b">a\nAC\n>b\nGT\n", 1, shift=shift)


def test_pairs_with_an_odd_count(db):
    rng = np.random.default_rng(31)
    T = api.parse_tile()
    for fq in (False, True):
        rec = fastq_record if fq else fasta_record
        data = b"".join(rec(b"p%d" % i, dna(rng, 90 + i)) for i in range(61))     # more than one tile
        assert len(data) > T
        closed = check(db, data, 4, pairs=True, what="pairs, closed, odd")
        assert closed.half == 1 and closed.whole == 61
        opened = check(db, data, 4, pairs=True, open_end=True, what="pairs, open, odd")
        assert opened.whole == 60 and opened.half == 0
        check(db, data, 62, pairs=True)
        check(db, data, 60, pairs=True, open_end=True)


@pytest.mark.parametrize("shift", [0, 1])
def test_a_range_of_two_to_the_31_bytes(db, shift):
    """the largest range the call takes: positions up to 2^31 - 1, tile starts up to 2^31.  2^25 records of 64 bytes, so the cuts are sums"""
    import torch
    dev = torch.device("cuda", 0)
    rec = b">r\n" + b"A" * 60 + b"\n"
    n, recs, R = 1 << 31, 1 << 25, 1 << 20
    assert len(rec) == 64 and recs * 64 == n
    buf = torch.full((n + 32,), 10, dtype=torch.uint8, device=dev)
    buf[shift:shift + n] = torch.from_numpy(np.frombuffer(rec, dtype=np.uint8).copy()).to(dev).repeat(recs)
    cuts = torch.full((GUARD + 33 + GUARD,), FILL64, dtype=torch.int64, device=dev)
    status = torch.full((8,), FILL64, dtype=torch.int64, device=dev)
    wsb = api.parse_cut_scratch_bytes(n)
    ws = torch.full((wsb + GUARD,), FILL, dtype=torch.uint8, device=dev)
    for open_end in (False, True):
        db.parse_cut_device(buf.data_ptr() + shift, n, R, cuts_ptr=cuts.data_ptr() + 8 * GUARD, capacity=33, status_ptr=status.data_ptr(),
                            workspace_ptr=ws.data_ptr(), workspace_bytes=wsb, open=open_end)
        torch.cuda.synchronize()
        whole, consumed = (recs - 1, n - 64) if open_end else (recs, n)
        assert [int(x) for x in status.cpu().numpy().view(np.uint64)] == [whole, 32, consumed, recs, 0, 0, R * 64, 0]
        c = cuts.cpu().numpy()
        assert np.all(c[:GUARD] == FILL64) and np.all(c[GUARD + 33:] == FILL64) and np.all(ws[wsb:].cpu().numpy() == FILL)
        assert [int(x) for x in c[GUARD:GUARD + 33]] == [i * R * 64 for i in range(32)] + [consumed]
    del buf


def test_capacity_one_short(db):
    data, _ = cases()["cli_reads.fa"]
    want = cut_ref.cut(data, 3)
    nb = len(want.cuts) - 1
    st, cuts = OnDevice(data, nb).enqueue(db, 3).result()
    assert st[:6] == [want.whole, nb, want.consumed, want.seen, api.PARSE_OVERFLOW, 0] and st[6] == 0
    assert np.all(cuts.view(np.int64) == FILL64), "cuts written with MC_PARSE_OVERFLOW"
    h = db.parse_cut(data, 3, capacity=nb)
    assert [int(x) for x in h["status"][:6]] == st[:6] and not h["raw"].any()
    h = db.parse_cut(data, 3)                                        # the second call takes nb from the first
    assert [int(x) for x in h["cuts"]] == want.cuts
    assert OnDevice(data, 0).enqueue(db, 3).result()[0][4] == api.PARSE_OVERFLOW


def test_two_streams_at_once(db):
    import torch
    names = ["cli_reads.fa", "cli_pairs.fq", "long_record_fa", "marker_at_T_fq", "header_across_fa_crlf", "fq_tail_2_lines"]
    streams = [torch.cuda.Stream(device=torch.device("cuda", 0)) for _ in range(2)]
    calls = []
    for k, name in enumerate(names * 2):
        data, pairs = cases()[name]
        calls.append((name, OnDevice(data, len(data) // 2 + 2), cut_ref.cut(data, 2, pairs, bool(k & 1)), pairs, bool(k & 1)))
    for k, (name, d, want, pairs, open_end) in enumerate(calls):
        d.enqueue(db, 2, pairs, open_end, stream=streams[k % 2].cuda_stream)
    for s in streams:
        s.synchronize()
    for name, d, want, pairs, open_end in calls:
        st, cuts = d.result()
        assert st[4] == want.verdict == parse_ref.OK and st[:4] == [want.whole, len(want.cuts) - 1, want.consumed, want.seen] and st[6] == want.longest, name
        assert [int(x) for x in cuts[:len(want.cuts)]] == want.cuts, name


def test_a_batch_cut_again_is_a_refinement(db):
    data, _ = cases()["cli_reads.fa"]
    first = check(db, data, 8, what="first cut")
    finer = []
    for a, b in zip(first.cuts, first.cuts[1:]):
        again = check(db, data[a:b], 4, shift=a % 16, what=f"batch at {a}")
        assert again.verdict == parse_ref.OK and again.cuts[0] == 0 and again.cuts[-1] == b - a and len(again.cuts) <= 3
        assert again.longest <= first.longest
        finer += [a + x for x in again.cuts[:-1]]
    finer.append(first.cuts[-1])
    assert finer == cut_ref.cut(data, 4).cuts and set(first.cuts) <= set(finer)


def test_chain_behind_the_device_inflate(db):
    """inflate -> cut on one stream, nothing waited for in between"""
    import torch
    plain, _ = cases()["cli_pairs.fq"]
    data = inflate_cases.bgzf_file(plain, payload=3000)
    rows, out_bytes, verdict, _ = inflate_ref.walk(data)
    assert verdict == inflate_ref.BGZF_OK and out_bytes == len(plain) and len(rows) > 4
    dev = torch.device("cuda", 0)
    padded = np.zeros((len(data) + 31) // 16 * 16, dtype=np.uint8)
    padded[:len(data)] = np.frombuffer(data, dtype=np.uint8)
    d_in = torch.from_numpy(padded).to(dev)
    d_rows = torch.from_numpy(np.array(rows, dtype=api.bgzf_block_dtype).view(np.uint8).copy()).to(dev)
    d_st = torch.zeros(4, dtype=torch.int64, device=dev)
    want = cut_ref.cut(plain, 6, pairs=True)
    c = OnDevice(b"\n" * out_bytes, len(want.cuts))                  # (the range is filled by the inflate)
    s = torch.cuda.Stream(device=dev)
    db.inflate_device(d_in.data_ptr(), len(data), d_rows.data_ptr(), len(rows), c.ptr(), out_bytes, d_st.data_ptr(), stream=s.cuda_stream)
    c.enqueue(db, 6, pairs=True, stream=s.cuda_stream)
    s.synchronize()
    assert [int(x) for x in d_st.cpu().numpy()] == [0, 0, 0, out_bytes]
    st, cuts = c.result()
    assert st == [want.whole, len(want.cuts) - 1, want.consumed, want.seen, 0, 0, want.longest, want.half]
    assert [int(x) for x in cuts] == want.cuts


# ---- mc_parse_headers -----------------------------------------------------------------------------------------------------------------------
def headers_on_device(db, data, hdr, parse_status, max_records, out_capacity, tail=b""):
    """the device form -> (status [4], out [out_capacity], out_off [max_records + 1]) as they lie in memory, guard zones checked"""
    import torch
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)
    d_bytes = up(np.frombuffer(b"\n" + data + tail, dtype=np.uint8))    # (bytes at an odd address; tail: what lies behind the range)
    d_hdr = up(np.concatenate([np.asarray(hdr, dtype=np.uint32).reshape(-1), np.zeros(4, dtype=np.uint32)]))
    d_ps = up(np.asarray(parse_status, dtype=np.uint64))
    out = torch.full((GUARD + out_capacity + GUARD,), FILL, dtype=torch.uint8, device=dev)
    off = torch.full((GUARD + max_records + 1 + GUARD,), FILL64, dtype=torch.int64, device=dev)
    status = torch.full((GUARD + 4 + GUARD,), FILL64, dtype=torch.int64, device=dev)
    wsb = api.parse_headers_scratch_bytes(max_records)
    ws = torch.full((wsb + GUARD,), FILL, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    db.parse_headers_device(d_bytes.data_ptr() + 1, len(data), hdr_ptr=d_hdr.data_ptr(), parse_status_ptr=d_ps.data_ptr(), max_records=max_records,
                            out_ptr=out.data_ptr() + GUARD, out_capacity=out_capacity, out_off_ptr=off.data_ptr() + 8 * GUARD, status_ptr=status.data_ptr() + 8 * GUARD,
                            workspace_ptr=ws.data_ptr(), workspace_bytes=wsb)
    torch.cuda.synchronize()
    out, off, status, ws = (t.cpu().numpy() for t in (out, off, status, ws))
    assert np.all(out[:GUARD] == FILL) and np.all(out[GUARD + out_capacity:] == FILL), "bytes outside out were written"
    assert np.all(off[:GUARD] == FILL64) and np.all(off[GUARD + max_records + 1:] == FILL64), "words outside out_off were written"
    assert np.all(status[:GUARD] == FILL64) and np.all(status[GUARD + 4:] == FILL64) and np.all(ws[wsb:] == FILL)
    return [int(x) for x in status[GUARD:GUARD + 4].view(np.uint64)], out[GUARD:GUARD + out_capacity], off[GUARD:GUARD + max_records + 1].view(np.uint64)


def check_headers(db, data, parsed, records, what):
    """the headers of the first `records` records (an hdr slice, parse_status[0] = records), both forms"""
    hdr = np.array([[r[0], r[1]] for r in parsed.records[:records]], dtype=np.uint32).reshape(records, 2)
    ps = np.array([records, records, 0, 0, parse_ref.OK, 0, 0, 0], dtype=np.uint64)
    text, off = cut_ref.headers(data, parse_ref.Parsed(parsed.verdict, 0, parsed.records[:records]))
    st, out, out_off = headers_on_device(db, data, hdr, ps, records, len(text))
    assert st == [records, len(text), parse_ref.OK, 0], f"{what}: {st}"
    assert out.tobytes() == text and [int(x) for x in out_off] == off, what
    h = db.parse_headers(data, hdr, ps)
    assert [int(x) for x in h["status"]] == [records, len(text), parse_ref.OK, 0] and h["out"] == text and [int(x) for x in h["out_off"]] == off, what
    return hdr, ps, text, off


HEADER_FILE = {}


def header_file():
    """65 537 short records; the first headers differ in length, one is empty, one lies across the tile border"""
    if not HEADER_FILE:
        T = api.parse_tile()
        rng = np.random.default_rng(41)
        head = pad_to(0, T - 10, rng, False) + fasta_record(b"x" * 30, dna(rng, 50), comment=b" across the border") + b">\nAC\n"
        n_head = len(parse_ref.parse(head).records)
        data = head + b"".join(b">h%d %s\nAC\n" % (i, b"w" * (i % 7)) for i in range(65537 - n_head))
        parsed = parse_ref.parse(data)
        assert parsed.verdict == parse_ref.OK and len(parsed.records) == 65537
        assert any(r[0] < T < r[0] + r[1] for r in parsed.records) and any(r[1] == 0 for r in parsed.records)
        HEADER_FILE.update(data=data, parsed=parsed)
    return HEADER_FILE["data"], HEADER_FILE["parsed"]


@pytest.mark.parametrize("records", [0, 1, 255, 256, 257, 65537])
def test_headers_against_the_model(db, records):
    data, parsed = header_file()
    check_headers(db, data, parsed, records, f"{records} records")


def test_headers_behind_the_parse_and_refusals(db):
    data, _ = cases()["header_across_fa_crlf"]
    got = db.parse_records(data)
    parsed = parse_ref.parse(data)
    assert int(got["status"][4]) == api.PARSE_OK
    text, off = cut_ref.headers(data, parsed)
    h = db.parse_headers(data, got["hdr"], got["status"])
    assert h["out"] == text and [int(x) for x in h["out_off"]] == off
    n = len(parsed.records)
    hdr, ps, text, off = check_headers(db, data, parsed, n, "every record")
    # a capacity one short: OVERFLOW, the bytes needed, nothing written
    st, out, out_off = headers_on_device(db, data, hdr, ps, n, len(text) - 1)
    assert st == [n, len(text), api.PARSE_OVERFLOW, 0] and np.all(out == FILL) and np.all(out_off.view(np.int64) == FILL64)
    h = db.parse_headers(data, hdr, ps, out_capacity=len(text) - 1)
    assert [int(x) for x in h["status"]] == [n, len(text), api.PARSE_OVERFLOW, 0] and not h["raw"][0].any() and not h["raw"][1].any()
    # more records than the arrays take
    st, out, out_off = headers_on_device(db, data, hdr, ps, n - 1, len(text))
    assert st == [n, 0, api.PARSE_OVERFLOW, 0] and np.all(out == FILL) and np.all(out_off.view(np.int64) == FILL64)
    # a parse that refused: its verdict passed through, nothing written
    for verdict in (api.PARSE_IRREGULAR, api.PARSE_OVERFLOW):
        bad = ps.copy()
        bad[4] = verdict
        st, out, out_off = headers_on_device(db, data, hdr, bad, n, len(text))
        assert st == [0, 0, verdict, 0] and np.all(out == FILL) and np.all(out_off.view(np.int64) == FILL64)
        assert [int(x) for x in db.parse_headers(data, hdr, bad)["status"]] == [0, 0, verdict, 0]


def test_header_rows_that_leave_the_range_read_nothing_outside_it(db):
    """hdr rows that are not this range's (a stale array): the copy stops at the end of the range"""
    data = b">abc\nAC\n"
    hdr = np.array([[1, 3], [6, 10], [40, 5]], dtype=np.uint32)
    ps = np.array([3, 3, 0, 0, parse_ref.OK, 0, 0, 0], dtype=np.uint64)
    st, out, out_off = headers_on_device(db, data, hdr, ps, 3, 18, tail=b"X" * 64)
    assert st == [3, 18, parse_ref.OK, 0] and [int(x) for x in out_off] == [0, 3, 13, 18]
    assert out[:5].tobytes() == b"abc" + data[6:8] and np.all(out[5:] == FILL), out.tobytes()
    h = db.parse_headers(data, hdr, ps, out_capacity=18)          # (the host form stages no more of out than the range has bytes: these rows do not fit)
    assert [int(x) for x in h["status"]] == [3, 18, api.PARSE_OVERFLOW, 0] and not h["raw"][0].any()


# ---- the slot that takes device bytes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pairs", [("cli_reads.fa", False), ("cli_pairs.fq", True)])
def test_query_device_bytes_equals_query_file_bytes(name, pairs):
    import torch
    d = api.Database.open(os.path.join(GOLDEN, "toy32"), max_candidates=2, copy_allhits=1)
    try:
        data = parse_cases.golden_bytes(name)
        dev_bytes = torch.from_numpy(np.frombuffer(b"\n" * 3 + data, dtype=np.uint8).copy()).to(torch.device("cuda", 0))
        base = dev_bytes.data_ptr() + 3                              # (the file at an odd address; its batches wherever their records begin)
        cuts = [int(x) for x in d.parse_cut(data, 24, pairs=pairs)["cuts"]]
        assert len(cuts) > 2 and any((base + c) % 16 for c in cuts)
        insert_max = 300 if pairs else 0
        for a, b in zip(cuts, cuts[1:]):
            want = d.query_file_bytes(data[a:b], pairs=pairs, insert_max=insert_max)
            got = d.query_device_bytes(base + a, b - a, pairs=pairs, insert_max=insert_max)
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (name, a)
            assert all(np.array_equal(x, y) for x, y in zip(got[2], want[2])) and len(got[2]) == len(want[2])
            for key in ("verdict", "offence", "records", "queries", "half_pair"):
                assert got[3][key] == want[3][key], (name, a, key)
            assert got[3]["verdict"] == api.PARSE_OK and got[3]["records"] == min(24, len(parse_ref.parse(data).records) - 24 * cuts.index(a))
            assert np.array_equal(got[3]["hdr"], want[3]["hdr"]) and np.array_equal(got[3]["qinfo"], want[3]["qinfo"])
            piece = data[a:b]
            assert got[3]["headers"] == [piece[h:h + l] for h, l, _ in parse_ref.parse(piece).records], (name, a)
    finally:
        d.close()


def test_device_slot_states_and_refused_ranges():
    import torch
    d = api.Database.open(os.path.join(GOLDEN, "toy32"), max_candidates=2, slot_max_chars=8192, slot_max_queries=16)
    L = api.lib()
    try:
        rng = np.random.default_rng(9)
        good = b"".join(fasta_record(b"r%d x" % i, dna(rng, 150), 60) for i in range(12))
        bad = good + b"+stray\n" + good[:200]
        dev = torch.from_numpy(np.frombuffer(b"\n" + good * 5 + bad, dtype=np.uint8).copy()).to(torch.device("cuda", 0))
        p_good, p_bad = dev.data_ptr() + 1, dev.data_ptr() + 1 + 5 * len(good)
        ref = d.query_file_bytes(good)
        heads = [good[h:h + l] for h, l, _ in parse_ref.parse(good).records]

        def same_as_ref():
            got = d.query_device_bytes(p_good, len(good))
            assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes() and got[3]["verdict"] == api.PARSE_OK and got[3]["headers"] == heads

        same_as_ref()
        assert L.mc_batch_add_device_bytes(d.h, 0, p_good, 5 * len(good), 0, 0) == api.MC_BATCH_FULL
        with pytest.raises(api.McError):
            d.query_device_bytes(p_good, 5 * len(good))
        same_as_ref()                                               # the slot is used again after MC_BATCH_FULL
        assert L.mc_batch_add_device_bytes(d.h, 0, p_good, len(good), 0, 0) == 0
        assert L.mc_batch_add_device_bytes(d.h, 0, p_good, len(good), 0, 0) == -6 and L.mc_batch_add(d.h, 0, b"ACGT" * 40, 160, b"", 0, 4) == -6
        text, off, n = api.C.c_void_p(), api.C.c_void_p(), api.C.c_uint64()
        assert L.mc_batch_headers(d.h, 0, api.C.byref(text), api.C.byref(off), api.C.byref(n)) == -6      # not submitted
        assert L.mc_batch_clear(d.h, 0) == 0
        assert L.mc_batch_add_device_bytes(d.h, 0, p_good, len(good), 4, 0) == -1 and L.mc_batch_add_device_bytes(d.h, 0, None, 5, 0, 0) == -1
        # a slot filled with host bytes has no header views
        buf = np.frombuffer(good, dtype=np.uint8)
        assert L.mc_batch_add_file_bytes(d.h, 0, buf.ctypes.data, len(buf), 0, 0) == 0 and L.mc_batch_submit(d.h, 0, 0) == 0
        res = api.McResults()
        assert L.mc_batch_wait(d.h, 0, api.C.byref(res)) == 0
        assert L.mc_batch_headers(d.h, 0, api.C.byref(text), api.C.byref(off), api.C.byref(n)) == -6
        assert L.mc_batch_clear(d.h, 0) == 0
        # an irregular range: no queries, no views
        cands, counts, _, rec = d.query_device_bytes(p_bad, len(bad))
        assert len(cands) == 0 and (rec["verdict"], rec["offence"], rec["records"]) == (api.PARSE_IRREGULAR, len(good), 0) and rec["headers"] is None
        same_as_ref()
    finally:
        d.close()


# ---- a file resident on the device (mc_input_*): what `mcq query` stands on ------------------------------------------------------------------
@pytest.mark.parametrize("name,pairs", [("cli_reads.fa", False), ("cli_pairs.fq", True)])
@pytest.mark.parametrize("packed", [False, True])
def test_resident_input_gives_the_batches_of_the_file(db, name, pairs, packed):
    """pieces of 3000 bytes chained by `consumed`; a slot of 2000 bytes, so that batches of 24 records are cut again (a refinement)"""
    plain = parse_cases.golden_bytes(name)
    data = inflate_cases.bgzf_file(plain, payload=3000) if packed else plain
    want = parse_ref.parse(plain).records
    res = db.resident_input(data, 24, pairs=pairs, piece_bytes=3000, slot_bytes=2000)
    try:
        info = [int(x) for x in res["info"]]
        assert info[:3] == [api.INPUT_OK, 0, len(plain)] and info[3] > len(plain) // 3000 and info[5] == len(want) and info[6] == int(packed)
        rows = res["batches"]
        assert info[4] == len(rows) and res["nbytes"] == len(plain) and res["handle"]
        assert db.download_input(res["handle"], res["nbytes"]) == plain                  # (BGZF: what the device inflated)
        at, got = 0, []
        for r in rows:
            assert int(r["offset"]) == at and (int(r["nbytes"]) <= 2000 or int(r["records"]) == (2 if pairs else 1)) and int(r["too_big"]) == int(int(r["nbytes"]) > 2000)
            p = parse_ref.parse(plain[at:at + int(r["nbytes"])])
            assert p.verdict == parse_ref.OK and len(p.records) == int(r["records"]) <= 24 and int(r["queries"]) == -(-len(p.records) // (2 if pairs else 1))
            got += [(at + h, l, s) for h, l, s in p.records]
            at += int(r["nbytes"])
        assert at == len(plain) and got == want and not rows["half_pair"].any()
        assert len(rows) > -(-len(want) // 24)                                            # some batch was cut again
        # a batch straight into a slot, from wherever it begins
        r = rows[len(rows) // 2]
        a, n = int(r["offset"]), int(r["nbytes"])
        dev, host = db.query_device_bytes(res["ptr"] + a, n, pairs=pairs), db.query_file_bytes(plain[a:a + n], pairs=pairs)
        assert dev[0].tobytes() == host[0].tobytes() and dev[3]["records"] == int(r["records"])
    finally:
        db.close_input(res["handle"])


def test_resident_input_refusals(db):
    fa = parse_cases.golden_bytes("cli_irregular.fa")
    offence = parse_ref.parse(fa).offence
    res = db.resident_input(fa, 23, piece_bytes=3000)
    assert [int(x) for x in res["info"][:2]] == [api.INPUT_IRREGULAR, offence] and not res["handle"]
    res = db.resident_input(inflate_cases.bgzf_file(fa, payload=3000), 23, piece_bytes=3000)
    try:                                                            # inflated there: the handle stays for the one copy back
        assert [int(x) for x in res["info"][:2]] == [api.INPUT_IRREGULAR, offence] and res["handle"] and len(res["batches"]) == 0
        assert db.download_input(res["handle"], res["nbytes"]) == fa
    finally:
        db.close_input(res["handle"])
    import gzip
    res = db.resident_input(gzip.compress(fa), 23)
    assert [int(x) for x in res["info"][:2]] == [api.INPUT_NOT_BGZF, 0] and not res["handle"]
    good = parse_cases.golden_bytes("cli_reads.fa")
    res = db.resident_input(good, 23, max_resident_bytes=len(good) - 1)
    assert int(res["info"][0]) == api.INPUT_TOO_LARGE and not res["handle"]
    odd = parse_cases.golden_bytes("cli_pairs.fq")
    odd = odd[:parse_ref.parse(odd).records[-1][0] - 1]            # without its last record: an odd number
    res = db.resident_input(odd, 4, pairs=True, piece_bytes=3000)
    try:
        assert int(res["info"][0]) == api.INPUT_OK and int(res["info"][5]) & 1 and list(res["batches"]["half_pair"]) == [0] * (len(res["batches"]) - 1) + [1]
    finally:
        db.close_input(res["handle"])
