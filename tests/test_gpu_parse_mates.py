"""GPU: mc_parse_mates (parse.hip), the device form and MC_PARSE_HOST, against the mates rule in plain Python (parse_mates_ref), and
the slot path mc_batch_add_file_mates against mc_batch_add and the C oracle.

The cases (parse_mates_cases) put record borders, a header and a long record at the tile T in one range only, one tile beside more
than 256, all 16 combinations of len1 % 4 / len2 % 4, FASTA beside FASTQ, '\\r\\n' or a missing final newline in one range only, and
query counts around a block (256) and a trip (65 536) of the per-record scan.  Every output lies between two guard zones.  A regular
input that the device refuses FAILS here: there is no skip and no fall-back."""
import os

import numpy as np
import pytest

import parse_cases
import parse_mates_cases
import parse_mates_ref as mref
import parse_ref
from parse_cases import dna, fasta_record, fastq_record, golden_bytes
from metacache_amd import api

pytestmark = pytest.mark.gpu
GOLDEN = parse_cases.GOLDEN
GUARD, FILL = 64, 0xA5
KEYS = ("hdr", "qinfo", "seq", "names", "name_off", "max_win")


@pytest.fixture(scope="module")
def db():
    d = api.Database.open(os.path.join(GOLDEN, "toy32"), max_candidates=3)
    yield d
    d.close()


CASES, WANT = None, {}


def cases():
    global CASES
    if CASES is None:
        CASES = parse_mates_cases.all_cases(api.parse_tile())
    return CASES


def want_of(db, name, insert_max=0):
    """the model's outputs for a case, computed once"""
    key = (name, insert_max)
    if key not in WANT:
        WANT[key] = mref.mates(*cases()[name], insert_max=insert_max, stride=db.stride)
        assert int(WANT[key]["status"][4]) == mref.OK, name
    return WANT[key]


def test_case_list_is_complete():
    assert sorted(cases()) == parse_mates_cases.CASE_NAMES


def assert_equal_to_model(got, want, what):
    st = [int(x) for x in got["status"]]
    assert st[4] == api.PARSE_OK, f"{what}: regular ranges were refused: status {st}"
    assert st == [int(x) for x in want["status"]], what
    for key in ("hdr", "qinfo", "name_off", "max_win"):
        assert np.array_equal(got[key], want[key]), (what, key)
    assert np.all(got["qinfo"][:, 0] % 4 == 0) and np.all(got["qinfo"][:, 2] % 4 == 0), what
    assert got["seq"] == want["seq"], what                       # (every mate's bytes, the padding and the 16 bytes behind the last)
    assert got["names"] == want["names"], what


class OnDevice:
    """two ranges and their outputs in device memory, every output between two guard zones"""

    def __init__(self, d1, d2, want_status, short=None):
        import torch
        self.torch, dev = torch, torch.device("cuda", 0)
        self.n = (len(d1), len(d2))
        self.bytes = [torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).to(dev) for d in (d1, d2)]
        recs, _, seq_need, name_need = (int(want_status[k]) for k in range(4))
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
        self.status = torch.full((10 + GUARD,), fill64, dtype=torch.int64, device=dev)
        self.ws_bytes = api.parse_mates_scratch_bytes(self.n[0], self.n[1], self.cap["max_records"])
        self.ws = torch.full((self.ws_bytes + GUARD,), FILL, dtype=torch.uint8, device=dev)
        assert all(b.data_ptr() % 16 == 0 for b in self.bytes) and self.seq.data_ptr() % 16 == 0 and self.ws.data_ptr() % 16 == 0
        torch.cuda.synchronize()

    def enqueue(self, db, insert_max=0, stream=0):
        db.parse_mates_device(self.bytes[0].data_ptr(), self.n[0], self.bytes[1].data_ptr(), self.n[1],
                              hdr_ptr=self.hdr.data_ptr() + 4 * GUARD, qinfo_ptr=self.qinfo.data_ptr() + 4 * GUARD,
                              seq_ptr=self.seq.data_ptr() + GUARD, seq_capacity=self.cap["seq"], names_ptr=self.names.data_ptr() + GUARD,
                              names_capacity=self.cap["names"], name_off_ptr=self.name_off.data_ptr() + 8 * GUARD, max_win_ptr=self.max_win.data_ptr() + 4 * GUARD,
                              status_ptr=self.status.data_ptr(), max_records=self.cap["max_records"], workspace_ptr=self.ws.data_ptr(),
                              workspace_bytes=self.ws_bytes, insert_max=insert_max, stream=stream)

    def arrays(self):
        self.torch.cuda.synchronize()
        host = lambda t, dt: t.cpu().numpy().view(dt)
        a = dict(hdr=host(self.hdr, np.uint32), qinfo=host(self.qinfo, np.uint32), seq=host(self.seq, np.uint8), names=host(self.names, np.uint8),
                 name_off=host(self.name_off, np.uint64), max_win=host(self.max_win, np.uint32), status=host(self.status, np.uint64), ws=host(self.ws, np.uint8))
        assert np.all(a["status"][10:].view(np.uint8) == FILL), "words behind status[10] were written"
        assert np.all(a["ws"][self.ws_bytes:] == FILL), "bytes behind the workspace were written"
        a["status"] = a["status"][:10]
        return a

    def result(self):
        """-> the outputs cut to what status reports; the guard zones must be untouched"""
        a = self.arrays()
        st = a["status"]
        r, q, sn, nn = (int(st[k]) for k in range(4))
        for key, used in (("hdr", 2 * r), ("qinfo", 4 * q), ("seq", sn), ("names", nn), ("name_off", q + 1), ("max_win", q)):
            raw = a[key].view(np.uint8)
            item = a[key].itemsize
            assert np.all(raw[:GUARD * item] == FILL), f"{key}: bytes in front of the array were written"
            assert np.all(raw[(GUARD + used) * item:] == FILL), f"{key}: bytes behind what status reports were written"
        cut = lambda key, used: a[key][GUARD:GUARD + used]
        return dict(status=st, hdr=cut("hdr", 2 * r).reshape(r, 2), qinfo=cut("qinfo", 4 * q).reshape(q, 4), seq=cut("seq", sn).tobytes(),
                    names=cut("names", nn).tobytes(), name_off=cut("name_off", q + 1), max_win=cut("max_win", q))

    def untouched(self):
        a = self.arrays()
        return all(np.all(a[k].view(np.uint8) == FILL) for k in KEYS)


@pytest.mark.parametrize("name", parse_mates_cases.CASE_NAMES)
def test_device_form_equals_the_model(db, name):
    want = want_of(db, name)
    d = OnDevice(*cases()[name], want["status"])
    d.enqueue(db)
    assert_equal_to_model(d.result(), want, name)


@pytest.mark.parametrize("name", [n for n in parse_mates_cases.CASE_NAMES if not n.startswith("count_6")])
def test_host_form_equals_the_model(db, name):
    want = want_of(db, name, insert_max=350)
    assert_equal_to_model(db.parse_mates(*cases()[name], insert_max=350), want, name)


@pytest.mark.parametrize("name", parse_mates_cases.FASTA_ONLY)
def test_two_fasta_ranges_equal_the_pairs_of_the_interleaved_file_on_the_device(db, name):
    d1, d2 = cases()[name]
    got = db.parse_mates(d1, d2, insert_max=200)
    pairs = db.parse_records(mref.interleave(d1, d2), pairs=True, insert_max=200)
    assert int(got["status"][4]) == int(pairs["status"][4]) == api.PARSE_OK
    assert [int(x) for x in got["status"][:7]] == [int(x) for x in pairs["status"][:7]]
    for key in ("qinfo", "name_off", "max_win"):
        assert np.array_equal(got[key], pairs[key]), key
    assert got["seq"] == pairs["seq"] and got["names"] == pairs["names"] and np.array_equal(got["hdr"][:, 1], pairs["hdr"][:, 1])


@pytest.mark.parametrize("longer", [0, 1])
def test_unequal_counts_are_refused_with_both_counts(db, longer):
    rng = np.random.default_rng(11)
    T = api.parse_tile()
    recs = [fasta_record(b"r%d" % i, dna(rng, 100 + i), 60) for i in range(2 * T // 100)]
    d = [b"".join(recs[:-1]), b"".join(recs[:-1])]
    d[longer] = b"".join(recs)
    n = [len(recs) - 1, len(recs) - 1]
    n[longer] += 1
    dev = OnDevice(d[0], d[1], [2 * len(recs), len(recs), len(d[0]) + len(d[1]) + 16, len(d[0])])
    dev.enqueue(db)
    st = [int(x) for x in dev.arrays()["status"]]
    assert (st[0], st[4], st[7], st[8], st[9]) == (n[0] + n[1], api.PARSE_UNEQUAL, 0, n[0], n[1]), st
    assert dev.untouched()
    want = [int(x) for x in mref.mates(d[0], d[1])["status"]]
    assert [st[k] for k in (0, 4, 7, 8, 9)] == [want[k] for k in (0, 4, 7, 8, 9)]
    got = db.parse_mates(d[0], d[1])
    assert [int(got["status"][k]) for k in (0, 4, 8, 9)] == [st[k] for k in (0, 4, 8, 9)] and "hdr" not in got


@pytest.mark.parametrize("where", ["range_2", "range_1", "both"])
def test_an_offence_names_its_range(db, where):
    rng = np.random.default_rng(12)
    T = api.parse_tile()
    good = parse_cases.pad_to(0, T + 200, rng, True)
    bad = good + b"stray\n" + fastq_record(b"b", b"ACGT")
    bad_early = fastq_record(b"a", b"ACGT") + b"@b\nACGT\nno plus\nIIII\n" + good
    d1, d2 = dict(range_2=(good, bad), range_1=(bad, good), both=(bad, bad_early))[where]
    want = [int(x) for x in mref.mates(d1, d2)["status"]]
    assert want[4] == mref.IRREGULAR and want[7] == (1 if where == "range_2" else 0) and want[5] == len(good)
    dev = OnDevice(d1, d2, [len(d1), len(d1), len(d1) + len(d2) + 16, len(d1)])
    dev.enqueue(db)
    st = [int(x) for x in dev.arrays()["status"]]
    assert (st[4], st[5], st[7]) == (api.PARSE_IRREGULAR, want[5], want[7]), st
    assert dev.untouched()
    got = db.parse_mates(d1, d2)
    assert [int(got["status"][k]) for k in (4, 5, 7)] == [st[k] for k in (4, 5, 7)] and "hdr" not in got


@pytest.mark.parametrize("short", ["max_records", "seq", "names"])
@pytest.mark.parametrize("name", ["lengths_mod_4", "header_across_in_2_fa"])
def test_overflow_reports_what_is_needed_and_writes_nothing(db, name, short):
    d1, d2 = cases()[name]
    want = want_of(db, name)
    kw = {("max_records" if short == "max_records" else short + "_capacity"): int(want["status"][dict(max_records=0, seq=2, names=3)[short]]) - 1}
    model = [int(x) for x in mref.mates(d1, d2, stride=db.stride, **kw)["status"]]
    d = OnDevice(d1, d2, want["status"], short=short)
    d.enqueue(db)
    st = [int(x) for x in d.arrays()["status"]]
    assert st[4] == api.PARSE_OVERFLOW and st == model, (name, short, st)
    assert d.untouched(), (name, short)
    d2nd = OnDevice(d1, d2, st)                                   # the second call, sized by the first one's status
    d2nd.enqueue(db)
    assert_equal_to_model(d2nd.result(), want, f"{name} after {short} overflow")
    caps = dict(max_records=int(want["status"][0]), seq_capacity=int(want["status"][2]), names_capacity=int(want["status"][3]))
    caps.update(kw)
    got = db.parse_mates(d1, d2, **caps)
    assert [int(x) for x in got["status"]] == model
    assert all(not np.any(v) for v in got["raw"].values()), (name, short)


def test_two_streams_at_once_and_the_same_call_twice(db):
    import torch
    names = ["one_tile_beside_many", "count_%d" % (parse_mates_cases.QUERY_TRIP + 1)]
    devs = [OnDevice(*cases()[n], want_of(db, n)["status"]) for n in names for _ in range(2)]
    streams = [torch.cuda.Stream(device=torch.device("cuda", 0)) for _ in range(2)]
    for k, d in enumerate(devs):
        d.enqueue(db, stream=streams[k % 2].cuda_stream)
    for st in streams:
        st.synchronize()
    results = [d.result() for d in devs]
    for k, n in enumerate(names):
        assert_equal_to_model(results[2 * k], want_of(db, n), f"{n} on stream 0")
        assert_equal_to_model(results[2 * k + 1], want_of(db, n), f"{n} on stream 1")
    # the same call again, on the same buffers: the same bytes, the workspace's included
    first = devs[0].arrays()
    devs[0].enqueue(db)
    again = devs[0].arrays()
    assert all(first[k].tobytes() == again[k].tobytes() for k in KEYS + ("status", "ws"))


def test_argument_errors_and_stats(db):
    import torch
    before = db.parse_stats()
    d1, d2 = cases()["single_query"]
    d = OnDevice(d1, d2, want_of(db, "single_query")["status"])
    L = api.lib()

    def call(p1=None, n1=len(d1), p2=None, n2=len(d2), flags=0, ws_bytes=None, seq_shift=0, status=True):
        o = api.McParseOutput(d.hdr.data_ptr(), d.qinfo.data_ptr(), d.seq.data_ptr() + seq_shift, 64, d.names.data_ptr(), 64, d.name_off.data_ptr(),
                              d.max_win.data_ptr(), d.status.data_ptr() if status else None, 2)
        return L.mc_parse_mates(db.h, d.bytes[0].data_ptr() if p1 is None else p1, n1, d.bytes[1].data_ptr() if p2 is None else p2, n2, flags, 0,
                                api.C.byref(o), d.ws.data_ptr(), d.ws_bytes if ws_bytes is None else ws_bytes, None)

    assert call(n1=1 << 30, n2=(1 << 30) + 1) == -1               # n1 + n2 > 2^31
    assert call(n1=0) == -1 and call(n2=0) == -1
    assert call(flags=api.PARSE_PAIRS) == -1 and call(flags=4) == -1
    assert call(p1=d.bytes[0].data_ptr() + 1) == -1 and call(p2=d.bytes[1].data_ptr() + 1) == -1   # misaligned inputs
    assert call(seq_shift=4) == -1
    assert call(ws_bytes=d.ws_bytes - 1) == -1
    assert call(status=False) == -1
    torch.cuda.synchronize()
    assert d.untouched() and np.all(d.arrays()["status"].view(np.uint8) == FILL)
    assert db.parse_stats() == before
    d.enqueue(db)
    d.result()
    after = db.parse_stats()
    assert [after[k] - before[k] for k in range(4)] == [1, len(d1) + len(d2), 2, 0]


# ---- two raw ranges into a batch slot (mc_batch_add_file_mates) ---------------------------------------------------------------------------
def assert_equal_to_oracle(odb, reads, mates, cands, counts, allhits, insert_max):
    assert len(cands) == len(reads)
    for i, r in enumerate(reads):
        h, c = odb.query(r, mates[i], 2, 0, insert_max)
        assert np.array_equal(allhits[i]["win"], h["win"]) and np.array_equal(allhits[i]["tgt"], h["tgt"]), i
        assert int(counts[i]) == len(h), i
        assert int((cands[i]["hits"] > 0).sum()) == len(c), i
        assert all(cands[i][j][f] == c[j][f] for j in range(len(c)) for f in ("tgt", "hits", "beg", "end")), i


def test_query_file_mates_equals_the_oracle_and_the_host_cut():
    import cpuref
    slot_db = api.Database.open(os.path.join(GOLDEN, "toy32"), max_candidates=2, copy_allhits=1)
    try:
        d1, d2 = golden_bytes("cli_p1.fa"), golden_bytes("cli_p2.fa")
        reads, mates = [r[2] for r in parse_ref.parse(d1).records], [r[2] for r in parse_ref.parse(d2).records]
        cands, counts, allhits, records = slot_db.query_file_mates(d1, d2, insert_max=300)
        want = mref.mates(d1, d2, insert_max=300, stride=slot_db.stride)
        assert (records["verdict"], records["records"], records["queries"], records["half_pair"]) == (api.PARSE_OK, 2 * len(reads), len(reads), 0)
        assert np.array_equal(records["hdr"], want["hdr"]) and np.array_equal(records["qinfo"], want["qinfo"])
        odb = cpuref.oracle().open(os.path.join(GOLDEN, "toy32"))
        try:
            assert_equal_to_oracle(odb, reads, mates, cands, counts, allhits, 300)
        finally:
            odb.close()
        hc, hn, hall = slot_db.query(reads, mates, insert_max=300)   # the same pairs through mc_batch_add
        assert hc.tobytes() == cands.tobytes() and hn.tobytes() == counts.tobytes()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(hall, allhits))
        # a refusal leaves no queries, and the slot works afterwards
        c2, n2, _, rec = slot_db.query_file_mates(d1, d2 + b">one more\nACGT\n", insert_max=300)
        assert len(c2) == 0 and len(n2) == 0 and (rec["verdict"], rec["records"], rec["queries"]) == (api.PARSE_UNEQUAL, 0, 0)
        c3, n3, _, _ = slot_db.query_file_mates(d1, d2, insert_max=300)
        assert c3.tobytes() == cands.tobytes() and n3.tobytes() == counts.tobytes()
    finally:
        slot_db.close()


def test_mates_slot_states():
    d = api.Database.open(os.path.join(GOLDEN, "toy32"), max_candidates=2, slot_max_chars=8192, slot_max_queries=16)
    L = api.lib()
    try:
        rng = np.random.default_rng(13)
        a = np.frombuffer(b"".join(fasta_record(b"r%d" % i, dna(rng, 150), 60) for i in range(12)), dtype=np.uint8)
        b = np.frombuffer(b"".join(fastq_record(b"r%d" % i, dna(rng, 100)) for i in range(12)), dtype=np.uint8)
        big = np.frombuffer(a.tobytes() * 4, dtype=np.uint8)
        assert len(a) + len(b) <= 8192 < len(big) + len(b)
        assert L.mc_batch_add_file_mates(d.h, 0, big.ctypes.data, len(big), b.ctypes.data, len(b), 0) == api.MC_BATCH_FULL
        assert L.mc_batch_add_file_mates(d.h, 0, None, 5, b.ctypes.data, len(b), 0) == -1 and L.mc_batch_add_file_mates(d.h, 0, a.ctypes.data, len(a), b.ctypes.data, 0, 0) == -1
        assert L.mc_batch_add_file_mates(d.h, 0, a.ctypes.data, len(a), b.ctypes.data, len(b), 0) == 0
        assert L.mc_batch_add_file_mates(d.h, 0, a.ctypes.data, len(a), b.ctypes.data, len(b), 0) == -6   # the slot holds ranges already
        assert L.mc_batch_clear(d.h, 0) == 0
        cands, counts, _, rec = d.query_file_mates(a.tobytes(), b.tobytes())
        assert rec["verdict"] == api.PARSE_OK and rec["queries"] == 12 and len(cands) == 12
        reads, mates = [r[2] for r in parse_ref.parse(a.tobytes()).records], [r[2] for r in parse_ref.parse(b.tobytes()).records]
        hc, hn, _ = d.query(reads, mates)
        assert hc.tobytes() == cands.tobytes() and hn.tobytes() == counts.tobytes()
        many = parse_mates_cases.tiny_records(17)                 # more pairs than slot_max_queries
        c2, _, _, rec = d.query_file_mates(many, many)
        assert len(c2) == 0 and rec["verdict"] == api.PARSE_OVERFLOW
        c3, _, _, rec = d.query_file_bytes(a.tobytes())           # a single range in the same slot afterwards
        assert rec["verdict"] == api.PARSE_OK and len(c3) == 12
    finally:
        d.close()
