"""GPU: mc_parse_records (parse.hip), the device form and MC_PARSE_HOST, against the record rule in plain Python (parse_ref).

  * the golden read files: every field of every record; the irregular ones get the irregular verdict and the model's offence;
  * generated files built around the tile T = api.parse_tile(): a marker at byte T, '\\n' at T - 1, '\\r' at T - 1 with '\\n' at T, a header
    across the border, the name's blank at T, one record of 2.5 T on lines of 60, more tiles than one trip of the scan of the tile sums
    takes (256), a single record, an empty sequence between two headers, no final newline, '>' and '@' inside sequence and quality
    lines, a quality line that starts with '@' -- each also with '\\r\\n' line ends;
  * pairs (even and odd counts), every capacity one short (outputs untouched, needs reported, the second call fits), two streams at once.
A regular input that the device refuses FAILS here: there is no skip and no fall-back."""
import os

import numpy as np
import pytest

import parse_cases
import parse_ref
from parse_cases import CASE_NAMES, IRREGULAR, REGULAR, fastq_record, golden_bytes, pad_to
from metacache_amd import api

pytestmark = pytest.mark.gpu
GOLDEN = parse_cases.GOLDEN
GUARD, FILL = 64, 0xA5


@pytest.fixture(scope="module")
def db():
    d = api.Database.open(os.path.join(GOLDEN, "toy32"), max_candidates=3)
    yield d
    d.close()


CASES = None


def cases():
    global CASES
    if CASES is None:
        CASES = parse_cases.all_cases(api.parse_tile())
    return CASES


def test_case_list_is_complete():
    assert sorted(CASE_NAMES) == sorted(cases())


# ---- comparison -----------------------------------------------------------------------------------------------------------------------
def assert_equal_to_model(got, data, want, what):
    st = [int(x) for x in got["status"]]
    assert st[4] == api.PARSE_OK, f"{what}: a regular range was refused: verdict {st[4]}, offence {st[5]}"
    assert st == [int(x) for x in want["status"]], what
    assert np.array_equal(got["hdr"], want["hdr"]), what
    assert np.array_equal(got["qinfo"], want["qinfo"]), what
    assert np.all(got["qinfo"][:, 0] % 4 == 0) and np.all(got["qinfo"][:, 2] % 4 == 0), what
    assert got["seq"] == want["seq"], what                       # (every read's bytes, the padding and the 16 bytes behind the last)
    q = got["qinfo"]
    for i in range(len(q)):
        for m in (0, 2):
            assert got["seq"][int(q[i, m]):int(q[i, m]) + int(q[i, m + 1])] == want["seq"][int(want["qinfo"][i, m]):int(want["qinfo"][i, m]) + int(q[i, m + 1])], (what, i)
    assert len(got["seq"]) >= (int(q[-1, 2]) + int(q[-1, 3]) if len(q) else 0) + 16, what
    assert got["names"] == want["names"] and np.array_equal(got["name_off"], want["name_off"]), what
    assert np.array_equal(got["max_win"], want["max_win"]), what


class OnDevice:
    """a range and its outputs in device memory, every output between two guard zones"""

    def __init__(self, data, want_status, short=None):
        import torch
        self.torch, dev = torch, torch.device("cuda", 0)
        n = len(data)
        self.n = n
        self.bytes = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev)
        recs, queries, seq_need, name_need = (int(want_status[k]) for k in range(4))
        self.cap = dict(max_records=recs, seq=seq_need, names=name_need)
        if short:
            self.cap[short] -= 1
        room = lambda elems: GUARD + elems + GUARD
        fill32 = int(np.array([FILL] * 4, dtype=np.uint8).view(np.int32)[0])
        fill64 = int(np.array([FILL] * 8, dtype=np.uint8).view(np.int64)[0])
        mr = recs
        self.hdr = torch.full((room(2 * mr),), fill32, dtype=torch.int32, device=dev)
        self.qinfo = torch.full((room(4 * mr),), fill32, dtype=torch.int32, device=dev)
        self.seq = torch.full((room(seq_need),), FILL, dtype=torch.uint8, device=dev)
        self.names = torch.full((room(name_need),), FILL, dtype=torch.uint8, device=dev)
        self.name_off = torch.full((room(mr + 1),), fill64, dtype=torch.int64, device=dev)
        self.max_win = torch.full((room(mr),), fill32, dtype=torch.int32, device=dev)
        self.status = torch.full((8,), fill64, dtype=torch.int64, device=dev)
        self.ws_bytes = api.parse_scratch_bytes(n)
        self.ws = torch.full((self.ws_bytes + GUARD,), FILL, dtype=torch.uint8, device=dev)
        assert self.bytes.data_ptr() % 16 == 0 and self.seq.data_ptr() % 16 == 0 and self.ws.data_ptr() % 16 == 0
        torch.cuda.synchronize()

    def enqueue(self, db, pairs=False, insert_max=0, stream=0):
        db.parse_device(self.bytes.data_ptr(), self.n, hdr_ptr=self.hdr.data_ptr() + 4 * GUARD, qinfo_ptr=self.qinfo.data_ptr() + 4 * GUARD,
                        seq_ptr=self.seq.data_ptr() + GUARD, seq_capacity=self.cap["seq"], names_ptr=self.names.data_ptr() + GUARD,
                        names_capacity=self.cap["names"], name_off_ptr=self.name_off.data_ptr() + 8 * GUARD, max_win_ptr=self.max_win.data_ptr() + 4 * GUARD,
                        status_ptr=self.status.data_ptr(), max_records=self.cap["max_records"], workspace_ptr=self.ws.data_ptr(),
                        workspace_bytes=self.ws_bytes, pairs=pairs, insert_max=insert_max, stream=stream)

    def arrays(self):
        self.torch.cuda.synchronize()
        host = lambda t, dt: t.cpu().numpy().view(dt)
        return dict(hdr=host(self.hdr, np.uint32), qinfo=host(self.qinfo, np.uint32), seq=host(self.seq, np.uint8), names=host(self.names, np.uint8),
                    name_off=host(self.name_off, np.uint64), max_win=host(self.max_win, np.uint32), status=host(self.status, np.uint64), ws=host(self.ws, np.uint8))

    def result(self):
        """-> the outputs cut to what status reports; the guard zones (and the workspace's) must be untouched"""
        a = self.arrays()
        st = a["status"]
        r, q, sn, nn = (int(st[k]) for k in range(4))
        for key, used in (("hdr", 2 * r), ("qinfo", 4 * q), ("seq", sn), ("names", nn), ("name_off", q + 1), ("max_win", q)):
            raw = a[key].view(np.uint8)
            item = a[key].itemsize
            assert np.all(raw[:GUARD * item] == FILL), f"{key}: bytes in front of the array were written"
            assert np.all(raw[(GUARD + used) * item:] == FILL), f"{key}: bytes behind what status reports were written"
        assert np.all(a["ws"][self.ws_bytes:] == FILL), "bytes behind the workspace were written"
        cut = lambda key, used: a[key][GUARD:GUARD + used]
        return dict(status=st, hdr=cut("hdr", 2 * r).reshape(r, 2), qinfo=cut("qinfo", 4 * q).reshape(q, 4), seq=cut("seq", sn).tobytes(),
                    names=cut("names", nn).tobytes(), name_off=cut("name_off", q + 1), max_win=cut("max_win", q))

    def untouched(self):
        a = self.arrays()
        return all(np.all(a[k].view(np.uint8) == FILL) for k in ("hdr", "qinfo", "seq", "names", "name_off", "max_win"))


WANT = {}


def want_of(db, name, pairs=False, insert_max=0):
    """the model's outputs for a case, computed once"""
    key = (name, pairs, insert_max)
    if key not in WANT:
        data = cases()[name]
        parsed = parse_ref.parse(data)
        assert parsed.verdict == parse_ref.OK, f"{name}: the model calls this input irregular at {parsed.offence}"
        WANT[key] = parse_ref.pack(data, parsed, pairs=pairs, insert_max=insert_max, stride=db.stride)
    return WANT[key]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_device_form_equals_the_model(db, name):
    data, want = cases()[name], want_of(db, name)
    d = OnDevice(data, want["status"])
    d.enqueue(db)
    assert_equal_to_model(d.result(), data, want, name)


@pytest.mark.parametrize("name", [n for n in CASE_NAMES if "many_tiles" not in n or n.endswith("_fa")])
def test_host_form_equals_the_model(db, name):
    data, want = cases()[name], want_of(db, name, insert_max=350)
    got = db.parse_records(data, insert_max=350)
    assert_equal_to_model(got, data, want, name)


@pytest.mark.parametrize("name", ["cli_pairs.fq", "cli_reads.fa", "long_record_fa", "long_record_fq_crlf", "header_across_fq", "single_fa", "blank_at_T_fa_crlf"])
def test_pairs(db, name):
    """cli_pairs.fq: 240 records = 120 pairs; long_record_*, single_*: an odd count, the last query is a half pair"""
    data, want = cases()[name], want_of(db, name, pairs=True, insert_max=200)
    if name in ("long_record_fa", "long_record_fq_crlf", "single_fa"):
        assert int(want["status"][7]) == 1 and int(want["qinfo"][-1, 3]) == 0
    d = OnDevice(data, want["status"])
    d.enqueue(db, pairs=True, insert_max=200)
    assert_equal_to_model(d.result(), data, want, name + " (device)")
    assert_equal_to_model(db.parse_records(data, pairs=True, insert_max=200), data, want, name + " (host)")


@pytest.mark.parametrize("name", IRREGULAR + ["plus_line_across_fa", "stray_line_fq", "incomplete_group_fq", "empty_sequence_fq", "no_marker"])
def test_irregular_ranges_are_refused_at_the_models_offence(db, name):
    T = api.parse_tile()
    rng = np.random.default_rng(8)
    if name in IRREGULAR:
        data = golden_bytes(name)
    elif name == "plus_line_across_fa":
        data = pad_to(0, T, rng, False) + b"+not a record\n>z\nACGT\n"
    elif name == "stray_line_fq":
        data = pad_to(0, T, rng, True) + fastq_record(b"a", b"ACGT") + b"stray\n" + fastq_record(b"b", b"ACGT")
    elif name == "incomplete_group_fq":
        data = fastq_record(b"a", b"ACGT") + b"@b\nACGT\n+\n"
    elif name == "empty_sequence_fq":
        data = fastq_record(b"a", b"ACGT") + b"@b\n\n+\n\n"
    else:
        data = b"ACGT\n>a\nACGT\n"
    parsed = parse_ref.parse(data)
    assert parsed.verdict == parse_ref.IRREGULAR
    d = OnDevice(data, [len(data), len(data), len(data) + 16, len(data)])
    d.enqueue(db)
    st = d.arrays()["status"]
    assert (int(st[4]), int(st[5])) == (api.PARSE_IRREGULAR, parsed.offence), name
    assert d.untouched(), name
    if name == "no_marker":
        with pytest.raises(api.McError):                          # (the host form reads the byte itself: an argument error)
            db.parse_records(data)
    else:
        got = db.parse_records(data)
        assert (int(got["status"][4]), int(got["status"][5])) == (api.PARSE_IRREGULAR, parsed.offence) and "hdr" not in got


@pytest.mark.parametrize("short", ["max_records", "seq", "names"])
@pytest.mark.parametrize("name", ["cli_reads.fa", "header_across_fq_crlf"])
def test_overflow_reports_what_is_needed_and_writes_nothing(db, name, short):
    data, want = cases()[name], want_of(db, name)
    d = OnDevice(data, want["status"], short=short)
    d.enqueue(db)
    st = [int(x) for x in d.arrays()["status"]]
    assert st[4] == api.PARSE_OVERFLOW and st[:4] == [int(x) for x in want["status"][:4]], (name, short, st)
    assert d.untouched(), (name, short)
    d2 = OnDevice(data, st)                                       # the second call, sized by the first one's status
    d2.enqueue(db)
    assert_equal_to_model(d2.result(), data, want, f"{name} after {short} overflow")
    # the host form: a capacity one short is reported, nothing is copied back
    caps = dict(max_records=int(want["status"][0]), seq_capacity=int(want["status"][2]), names_capacity=int(want["status"][3]))
    caps["max_records" if short == "max_records" else short + "_capacity"] -= 1
    got = db.parse_records(data, **caps)
    assert int(got["status"][4]) == api.PARSE_OVERFLOW and [int(x) for x in got["status"][:4]] == st[:4]
    assert all(not np.any(v) for v in got["raw"].values()), (name, short)


def test_two_streams_at_once(db):
    import torch
    names = ["many_tiles_fa", "many_tiles_fq_crlf"]
    devs = [OnDevice(cases()[n], want_of(db, n)["status"]) for n in names for _ in range(2)]
    streams = [torch.cuda.Stream(device=torch.device("cuda", 0)) for _ in range(2)]
    for k, d in enumerate(devs):
        d.enqueue(db, stream=streams[k % 2].cuda_stream)
    for st in streams:
        st.synchronize()
    results = [d.result() for d in devs]
    for k, n in enumerate(names):
        assert_equal_to_model(results[2 * k], cases()[n], want_of(db, n), f"{n} on stream 0")
        assert_equal_to_model(results[2 * k + 1], cases()[n], want_of(db, n), f"{n} on stream 1")
        for key in ("seq", "names"):
            assert results[2 * k][key] == results[2 * k + 1][key]


def test_argument_errors_and_stats(db):
    import torch
    dev = torch.device("cuda", 0)
    before = db.parse_stats()
    data = cases()["single_fa"]
    d = OnDevice(data, want_of(db, "single_fa")["status"])
    L = api.lib()

    def call(bytes_ptr=None, nbytes=len(data), flags=0, ws=None, ws_bytes=None, seq_shift=0, status=True):
        o = api.McParseOutput(d.hdr.data_ptr(), d.qinfo.data_ptr(), d.seq.data_ptr() + seq_shift, 64, d.names.data_ptr(), 64, d.name_off.data_ptr(),
                              d.max_win.data_ptr(), d.status.data_ptr() if status else None, 1)
        return L.mc_parse_records(db.h, d.bytes.data_ptr() if bytes_ptr is None else bytes_ptr, nbytes, flags, 0, api.C.byref(o),
                                  d.ws.data_ptr() if ws is None else ws, d.ws_bytes if ws_bytes is None else ws_bytes, None)

    assert call(nbytes=(1 << 31) + 1) == -1
    assert call(nbytes=0) == -1
    assert call(flags=4) == -1
    assert call(bytes_ptr=d.bytes.data_ptr() + 1) == -1           # misaligned input
    assert call(seq_shift=4) == -1                                # misaligned seq
    assert call(ws_bytes=d.ws_bytes - 1) == -1
    assert call(status=False) == -1
    torch.cuda.synchronize()
    assert d.untouched() and np.all(d.arrays()["status"].view(np.uint8) == FILL)
    assert db.parse_stats() == before
    d.enqueue(db)
    d.result()
    after = db.parse_stats()
    assert [after[k] - before[k] for k in range(4)] == [1, len(data), 1, 0]
    del dev


# ---- raw bytes into a batch slot (mc_batch_add_file_bytes) --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def slot_db():
    d = api.Database.open(os.path.join(GOLDEN, "toy32"), max_candidates=2, copy_allhits=1)
    yield d
    d.close()


def assert_equal_to_oracle(odb, reads, mates, cands, counts, allhits, insert_max):
    assert len(cands) == len(reads)
    for i, r in enumerate(reads):
        h, c = odb.query(r, mates[i] if mates is not None else b"", 2, 0, insert_max)
        assert np.array_equal(allhits[i]["win"], h["win"]) and np.array_equal(allhits[i]["tgt"], h["tgt"]), i
        assert int(counts[i]) == len(h), i
        assert int((cands[i]["hits"] > 0).sum()) == len(c), i
        assert all(cands[i][j][f] == c[j][f] for j in range(len(c)) for f in ("tgt", "hits", "beg", "end")), i


@pytest.mark.parametrize("name,pairs", [("cli_reads.fa", False), ("cli_pairs.fq", True)])
def test_query_file_bytes_equals_the_oracle_and_the_host_cut(slot_db, name, pairs):
    import cpuref
    data = golden_bytes(name)
    parsed = parse_ref.parse(data)
    reads, mates = parse_ref.reads_of(parsed, pairs)
    insert_max = 300 if pairs else 0
    cands, counts, allhits, records = slot_db.query_file_bytes(data, pairs=pairs, insert_max=insert_max)
    assert records["verdict"] == api.PARSE_OK and records["records"] == len(parsed.records) and records["queries"] == len(reads) and records["half_pair"] == 0
    want = parse_ref.pack(data, parsed, pairs=pairs, insert_max=insert_max, stride=slot_db.stride)
    assert np.array_equal(records["hdr"], want["hdr"]) and np.array_equal(records["qinfo"], want["qinfo"])
    odb = cpuref.oracle().open(os.path.join(GOLDEN, "toy32"))
    try:
        assert_equal_to_oracle(odb, reads, mates, cands, counts, allhits, insert_max)
    finally:
        odb.close()
    # the same reads cut on the host: byte for byte the same results
    hc, hn, hall = slot_db.query(reads, mates, insert_max=insert_max)
    assert hc.tobytes() == cands.tobytes() and hn.tobytes() == counts.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(hall, allhits))
    if not pairs:
        seqs = np.frombuffer(b"".join(reads), dtype=np.uint8)
        offs = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
        assert slot_db.query_bulk(seqs, offs).tobytes() == cands.tobytes()


def test_slot_states_and_refused_ranges():
    """MC_BATCH_FULL, a used slot, an irregular range, more reads than the slot takes -- and the slot works after each"""
    d = api.Database.open(os.path.join(GOLDEN, "toy32"), max_candidates=2, copy_allhits=1, slot_max_chars=8192, slot_max_queries=16)
    L = api.lib()
    try:
        rng = np.random.default_rng(9)
        good = b"".join(parse_cases.fasta_record(b"r%d x" % i, parse_cases.dna(rng, 150), 60) for i in range(12))
        ref = d.query_file_bytes(good)
        assert ref[3]["verdict"] == api.PARSE_OK and len(ref[0]) == 12

        def same_as_ref():
            got = d.query_file_bytes(good)
            assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes() and got[3]["verdict"] == api.PARSE_OK

        big = np.frombuffer(good * 5, dtype=np.uint8)
        assert len(big) > 8192
        assert L.mc_batch_add_file_bytes(d.h, 0, big.ctypes.data, len(big), 0, 0) == api.MC_BATCH_FULL
        with pytest.raises(api.McError):
            d.query_file_bytes(good * 5)
        same_as_ref()
        # a slot that holds reads, a raw slot that is given reads or a second range: MC_ERR_STATE, and what it held stays
        buf = np.frombuffer(good, dtype=np.uint8)
        assert L.mc_batch_add(d.h, 0, b"ACGT" * 40, 160, b"", 0, 4) == 0
        assert L.mc_batch_add_file_bytes(d.h, 0, buf.ctypes.data, len(buf), 0, 0) == -6
        assert L.mc_batch_clear(d.h, 0) == 0
        assert L.mc_batch_add_file_bytes(d.h, 0, buf.ctypes.data, len(buf), 0, 0) == 0
        assert L.mc_batch_add_file_bytes(d.h, 0, buf.ctypes.data, len(buf), 0, 0) == -6
        assert L.mc_batch_add(d.h, 0, b"ACGT" * 40, 160, b"", 0, 4) == -6
        info = api.McBatchRecordInfo()
        assert L.mc_batch_records(d.h, 0, api.C.byref(info)) == -6              # not submitted yet
        assert L.mc_batch_add_file_bytes(d.h, 0, buf.ctypes.data, len(buf), 4, 0) == -1 and L.mc_batch_add_file_bytes(d.h, 99, buf.ctypes.data, len(buf), 0, 0) == -1
        assert L.mc_batch_add_file_bytes(d.h, 0, None, 5, 0, 0) == -1
        assert L.mc_batch_clear(d.h, 0) == 0
        assert L.mc_batch_records(d.h, 0, api.C.byref(info)) == -6
        same_as_ref()
        # an irregular range: no queries, verdict and offence from mc_batch_records
        bad = good + b"+stray\n" + good[:200]
        cands, counts, _, rec = d.query_file_bytes(bad)
        assert len(cands) == 0 and len(counts) == 0 and (rec["verdict"], rec["offence"], rec["records"]) == (api.PARSE_IRREGULAR, len(good), 0)
        same_as_ref()
        # more reads than slot_max_queries, and a read of len + 8 > slot_max_chars: overflow, the caller takes the batch the old way
        many = b"".join(parse_cases.fasta_record(b"s%d" % i, b"ACGTACGTAC") for i in range(17))
        cands, _, _, rec = d.query_file_bytes(many)
        assert len(cands) == 0 and rec["verdict"] == api.PARSE_OVERFLOW
        same_as_ref()
        long_read = b">l\n" + parse_cases.dna(rng, 8188) + b"\n"
        assert len(long_read) == 8192
        cands, _, _, rec = d.query_file_bytes(long_read)
        assert len(cands) == 0 and rec["verdict"] == api.PARSE_OVERFLOW
        same_as_ref()
        st = d.parse_stats()
        assert st[0] >= 8 and st[3] == 2                          # (the irregular range and the 17 reads; the long read is refused on the host)
    finally:
        d.close()


def test_raw_slot_of_a_context_that_unites_its_slots():
    """small slots without all-hits lists are united by the coalescer; a raw slot goes alone and gives what the host cut gives"""
    d = api.Database.open(os.path.join(GOLDEN, "toy32"), max_candidates=2, num_slots=2, slot_max_queries=512, slot_max_chars=1 << 17)
    try:
        st = np.zeros(4, dtype=np.uint64)
        assert api.lib().mc_slot_stats(d.h, api.C.c_void_p(st.ctypes.data)) == 0 and int(st[0]) == 1
        data = golden_bytes("cli_reads.fa")
        reads, _ = parse_ref.reads_of(parse_ref.parse(data))
        cands, counts, _, rec = d.query_file_bytes(data, slot=1)
        assert rec["verdict"] == api.PARSE_OK and rec["queries"] == len(reads)
        hc, hn, _ = d.query(reads, slot=0)
        assert hc.tobytes() == cands.tobytes() and hn.tobytes() == counts.tobytes()
        cands2, _, _, _ = d.query_file_bytes(data, slot=0)
        assert cands2.tobytes() == cands.tobytes()
    finally:
        d.close()
