"""GPU: mc_parse_targets (parse_targets.hip), the device form and MC_PARSE_HOST, against the target rule in plain Python (targets_ref).

  * every regular case of targets_cases: hdr, targets and seq byte for byte (padding and the 16 zero bytes included) and status; the
    guard zones around every output and behind the workspace stay untouched;
  * irregular ranges, bad file tables and both kinds of MC_PARSE_OVERFLOW leave poisoned outputs untouched and report the model's status;
    the second call with what status asks for succeeds;
  * two runs on the same bytes are identical; mc_parse_headers behind the parse gives the model's headers; mc_parse_stats counts the calls;
  * end to end: parse_targets_device -> Builder.add_parsed_targets -> finish against the same records through Builder.add_target from
    host strings: the same features, location lists and window counts.
The context is one WITHOUT a database (Database.create).  A regular input that the device refuses FAILS here."""
import ctypes as C

import numpy as np
import pytest

import targets_cases
import targets_ref
from targets_cases import BAD_TABLE_NAMES, IRREGULAR_NAMES, REGULAR_NAMES
from metacache_amd import api

pytestmark = pytest.mark.gpu
GUARD, FILL = 64, 0xA5
TSIZE = targets_ref.target_dtype.itemsize


@pytest.fixture(scope="module")
def db():
    d = api.Database.create()
    yield d
    d.close()


CASES, WANT = {}, {}


def regular():
    if "regular" not in CASES:
        CASES["regular"] = targets_cases.regular_cases(api.parse_tile())
    return CASES["regular"]


def want_of(name):
    """the model's outputs for a regular case, computed once"""
    if name not in WANT:
        parsed = targets_ref.parse(regular()[name])
        assert parsed.verdict == targets_ref.OK, f"{name}: the model calls this input irregular at {parsed.offence}"
        WANT[name] = (parsed, targets_ref.pack(parsed))
    return WANT[name]


def test_the_api_record_is_the_models():
    assert api.parse_target_dtype == targets_ref.target_dtype and C.sizeof(api.McParseTargetsOutput) == 48


class OnDevice:
    """a range, its file table and its outputs in device memory, every output between two guard zones"""

    def __init__(self, data, file_off, max_records, seq_capacity):
        import torch
        self.torch, dev = torch, torch.device("cuda", 0)
        self.n, self.files = len(data), len(file_off) - 1
        self.bytes = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev)
        self.file_off = torch.from_numpy(np.ascontiguousarray(file_off, dtype=np.uint64).view(np.int64).copy()).to(dev)
        self.max_records, self.seq_capacity = max_records, seq_capacity
        fill32 = int(np.array([FILL] * 4, dtype=np.uint8).view(np.int32)[0])
        fill64 = int(np.array([FILL] * 8, dtype=np.uint8).view(np.int64)[0])
        self.hdr = torch.full((GUARD + 2 * max_records + GUARD,), fill32, dtype=torch.int32, device=dev)
        self.targets = torch.full((GUARD + TSIZE * max_records + GUARD,), FILL, dtype=torch.uint8, device=dev)
        self.seq = torch.full((GUARD + seq_capacity + GUARD,), FILL, dtype=torch.uint8, device=dev)
        self.status = torch.full((8,), fill64, dtype=torch.int64, device=dev)
        self.ws_bytes = api.parse_targets_scratch_bytes(self.n, self.files, max_records)
        self.ws = torch.full((self.ws_bytes + GUARD,), FILL, dtype=torch.uint8, device=dev)
        assert self.bytes.data_ptr() % 16 == 0 and self.seq.data_ptr() % 16 == 0 and self.ws.data_ptr() % 16 == 0 and self.targets.data_ptr() % 8 == 0
        torch.cuda.synchronize()

    def ptrs(self):
        return dict(hdr_ptr=self.hdr.data_ptr() + 4 * GUARD, targets_ptr=self.targets.data_ptr() + GUARD, seq_ptr=self.seq.data_ptr() + GUARD, status_ptr=self.status.data_ptr())

    def enqueue(self, db, stream=0):
        db.parse_targets_device(self.bytes.data_ptr(), self.n, self.file_off.data_ptr(), self.files, seq_capacity=self.seq_capacity, max_records=self.max_records,
                                workspace_ptr=self.ws.data_ptr(), workspace_bytes=self.ws_bytes, stream=stream, **self.ptrs())

    def arrays(self):
        self.torch.cuda.synchronize()
        host = lambda t, dt: t.cpu().numpy().view(dt)
        return dict(hdr=host(self.hdr, np.uint32), targets=host(self.targets, np.uint8), seq=host(self.seq, np.uint8), status=host(self.status, np.uint64), ws=host(self.ws, np.uint8))

    def result(self):
        """-> the outputs cut to what status reports; the guard zones (and the workspace's) must be untouched"""
        a = self.arrays()
        st = a["status"]
        r, sn = int(st[0]), int(st[2])
        for key, item, used in (("hdr", 4, 2 * r), ("targets", 1, TSIZE * r), ("seq", 1, sn)):
            raw = a[key].view(np.uint8)
            assert np.all(raw[:GUARD * item] == FILL), f"{key}: bytes in front of the array were written"
            assert np.all(raw[(GUARD + used) * item:] == FILL), f"{key}: bytes behind what status reports were written"
        assert np.all(a["ws"][self.ws_bytes:] == FILL), "bytes behind the workspace were written"
        return dict(status=st, hdr=a["hdr"][GUARD:GUARD + 2 * r].reshape(r, 2), targets=a["targets"][GUARD:GUARD + TSIZE * r].copy().view(targets_ref.target_dtype),
                    seq=a["seq"][GUARD:GUARD + sn].tobytes())

    def untouched(self):
        a = self.arrays()
        return all(np.all(a[k].view(np.uint8) == FILL) for k in ("hdr", "targets", "seq")) and np.all(a["ws"][self.ws_bytes:] == FILL)


def assert_equal_to_model(got, want, what):
    st = [int(x) for x in got["status"]]
    assert st[4] == api.PARSE_OK, f"{what}: a regular range was refused: verdict {st[4]}, offence {st[5]} in file {st[7]}"
    assert st == [int(x) for x in want["status"]], what
    assert np.array_equal(got["hdr"], want["hdr"]), what
    for field in ("seq_off", "len", "file", "index", "reserved"):
        assert np.array_equal(got["targets"][field], want["targets"][field]), (what, field)
    assert np.all(got["targets"]["seq_off"] % 4 == 0), what
    assert got["seq"] == want["seq"], what                       # (every sequence's bytes, the padding and the 16 bytes behind the last)


@pytest.mark.parametrize("name", REGULAR_NAMES)
def test_regular_case_device_and_host_form(db, name):
    files = regular()[name]
    data, off = b"".join(files), targets_ref.table_of(files)
    parsed, want = want_of(name)
    dev = OnDevice(data, off, int(want["status"][0]), int(want["status"][2]))
    dev.enqueue(db)
    assert_equal_to_model(dev.result(), want, name + " (device form)")
    assert_equal_to_model(db.parse_targets(data, off), want, name + " (host form)")


@pytest.mark.parametrize("name", IRREGULAR_NAMES)
def test_irregular_range_leaves_the_outputs_untouched(db, name):
    files, f, at = targets_cases.irregular_cases(api.parse_tile())[name]
    data, off = b"".join(files), targets_ref.table_of(files)
    want = targets_ref.pack(targets_ref.parse(files))["status"].tolist()
    assert want[4:] == [api.PARSE_IRREGULAR, int(off[f]) + at, 0, f]
    dev = OnDevice(data, off, 64, len(data) + 16)
    dev.enqueue(db)
    assert dev.untouched(), name
    assert dev.arrays()["status"].tolist() == want, name
    got = db.parse_targets(data, off, max_records=64, seq_capacity=len(data) + 16)
    assert got["status"].tolist() == want and "hdr" not in got and not got["raw"]["seq"].any() and not got["raw"]["hdr"].any(), name


@pytest.mark.parametrize("name", BAD_TABLE_NAMES)
def test_bad_file_table_is_found_on_the_device(db, name):
    data, off, row = targets_cases.bad_tables()[name]
    dev = OnDevice(data, off, 8, len(data) + 16)
    dev.enqueue(db)
    assert dev.untouched(), name
    assert dev.arrays()["status"].tolist() == [0, 0, 0, 0, api.PARSE_IRREGULAR, len(data), 0, row], name
    with pytest.raises(api.McError, match="file table"):         # the host form refuses it before any device call
        db.parse_targets(data, off)


@pytest.mark.parametrize("name", ["empty_records", "long_record_crlf", "tiny_files"])
@pytest.mark.parametrize("short", ["max_records", "seq"])
def test_overflow_reports_the_needs_and_the_second_call_fits(db, name, short):
    files = regular()[name]
    data, off = b"".join(files), targets_ref.table_of(files)
    parsed, want = want_of(name)
    recs, need = int(want["status"][0]), int(want["status"][2])
    cap = dict(max_records=recs, seq=need)
    cap[short] -= 1
    dev = OnDevice(data, off, cap["max_records"], cap["seq"])
    dev.enqueue(db)
    assert dev.untouched(), (name, short)
    st = dev.arrays()["status"].tolist()
    ws = want["status"].tolist()
    assert st == [ws[0], ws[1], ws[2], 0, api.PARSE_OVERFLOW, 0, ws[6], 0], (name, short)
    second = OnDevice(data, off, st[0], st[2])
    second.enqueue(db)
    assert_equal_to_model(second.result(), want, f"{name}: second call")
    # the host form: untouched arrays with the short capacity, and the two calls of its own where the capacities are left out
    got = db.parse_targets(data, off, max_records=cap["max_records"], seq_capacity=cap["seq"])
    assert got["status"].tolist() == st and not got["raw"]["seq"].any() and not got["raw"]["targets"].view(np.uint8).any(), (name, short)
    assert_equal_to_model(db.parse_targets(data, off), want, f"{name}: host form sized by status")


def test_no_room_at_all(db):
    files = regular()["blank_lines"]
    data, off = b"".join(files), targets_ref.table_of(files)
    _, want = want_of("blank_lines")
    dev = OnDevice(data, off, 0, 0)
    dev.enqueue(db)
    ws = want["status"].tolist()
    assert dev.untouched() and dev.arrays()["status"].tolist() == [ws[0], ws[1], ws[2], 0, api.PARSE_OVERFLOW, 0, ws[6], 0]


def test_two_runs_are_identical_and_streams_may_run_at_once(db):
    import torch
    files = regular()["many_tiles"]
    data, off = b"".join(files), targets_ref.table_of(files)
    _, want = want_of("many_tiles")
    runs = [OnDevice(data, off, int(want["status"][0]), int(want["status"][2])) for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in runs]
    for r, s in zip(runs, streams):
        r.enqueue(db, stream=s.cuda_stream)
    a, b = (r.arrays() for r in runs)
    for key in ("hdr", "targets", "seq", "status"):
        assert np.array_equal(a[key], b[key]), key
    assert_equal_to_model(runs[1].result(), want, "second stream")


def test_parse_headers_behind_the_parse(db):
    import torch
    for name in ("empty_records_crlf", "header_across_file_end", "golden_genomes"):
        files = regular()[name]
        data, off = b"".join(files), targets_ref.table_of(files)
        parsed, want = want_of(name)
        recs = int(want["status"][0])
        dev = OnDevice(data, off, recs, int(want["status"][2]))
        d = torch.device("cuda", 0)
        out = torch.zeros(len(data), dtype=torch.uint8, device=d)
        out_off = torch.zeros(recs + 1, dtype=torch.int64, device=d)
        hst = torch.zeros(4, dtype=torch.int64, device=d)
        hws_bytes = api.parse_headers_scratch_bytes(recs)
        hws = torch.zeros(hws_bytes, dtype=torch.uint8, device=d)
        dev.enqueue(db)
        db.parse_headers_device(dev.bytes.data_ptr(), dev.n, hdr_ptr=dev.ptrs()["hdr_ptr"], parse_status_ptr=dev.status.data_ptr(), max_records=recs, out_ptr=out.data_ptr(),
                                out_capacity=len(data), out_off_ptr=out_off.data_ptr(), status_ptr=hst.data_ptr(), workspace_ptr=hws.data_ptr(), workspace_bytes=hws_bytes)
        torch.cuda.synchronize()
        headers = targets_ref.headers_of(data, parsed)
        assert hst.cpu().numpy().view(np.uint64).tolist() == [recs, sum(len(h) for h in headers), api.PARSE_OK, 0], name
        o, text = out_off.cpu().numpy(), out.cpu().numpy().tobytes()
        assert [text[int(o[r]):int(o[r + 1])] for r in range(recs)] == headers, name
        # and the host forms one behind the other
        got = db.parse_targets(data, off)
        packed = db.parse_headers(data, got["hdr"], got["status"])
        assert [packed["out"][int(packed["out_off"][r]):int(packed["out_off"][r + 1])] for r in range(recs)] == headers, name


def test_parse_stats_count_the_calls_and_the_timers_have_their_names():
    files = regular()["long_record"]
    data, off = b"".join(files), targets_ref.table_of(files)
    _, want = want_of("long_record")
    d = api.Database.create()
    try:
        d.timing(True)
        assert d.parse_stats() == [0, 0, 0, 0]
        assert int(d.parse_targets(data, off)["status"][4]) == api.PARSE_OK        # two calls: the first reports the needs
        bad = targets_cases.irregular_cases(api.parse_tile())["plus_line"][0]
        assert int(d.parse_targets(b"".join(bad), targets_ref.table_of(bad))["status"][4]) == api.PARSE_IRREGULAR
        assert d.parse_stats() == [3, 2 * len(data) + len(b"".join(bad)), int(want["status"][0]), 2]
        for kernel, launches in (("targets_classify", 3), ("targets_write", 1)):   # (a call without room for a record has nothing to write)
            ms, count = d.timing_get(kernel)
            assert count == launches and ms > 0, kernel
    finally:
        d.close()


def target_windows(bld, t):
    n = C.c_uint64()
    L = api.lib()
    L.mc_build_target_windows.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    bld._check(L.mc_build_target_windows(bld.h, t, C.byref(n)))
    return n.value


def test_end_to_end_build_equals_the_build_from_host_strings(db):
    """parse_targets_device -> add_parsed_targets -> finish, against add_target with the model's sequences"""
    rng = np.random.default_rng(21)
    dna = targets_cases.dna
    files = [b"".join(targets_cases.fasta_record(b"t%d.%d desc" % (f, i), dna(rng, 700 + 331 * ((f + i) % 4)), 70) for i in range(1 + f % 3)) + (b">empty.%d\n" % f if f % 2 else b"")
             for f in range(5)]
    files[3] = files[3][:-1]                                     # (no final '\n')
    data, off = b"".join(files), targets_ref.table_of(files)
    parsed = targets_ref.parse(files)
    want = targets_ref.pack(parsed)
    recs = int(want["status"][0])
    names = [h.split(b" ")[0].decode() for h in targets_ref.headers_of(data, parsed)]
    filenames = [f"file{f}.fa" for f in range(len(files))]
    kw = dict(kmerlen=16, sketchlen=16, winlen=128, winstride=113, target_id_bytes=4, max_candidates=2)

    dev = OnDevice(data, off, recs, int(want["status"][2]))
    dev.enqueue(db)
    got = dev.result()
    assert_equal_to_model(got, want, "end to end")
    a, b = api.Builder(**kw), api.Builder(**kw)
    da = dbb = None
    try:
        added = a.add_parsed_targets(dev.ptrs()["seq_ptr"], got["targets"], names, [1000] * recs, filenames)
        assert added == int(want["status"][1]) < recs
        da = a.finish(load=True)
        for (_, _, seq, f, i), name in zip(parsed.records, names):
            if seq:
                b.add_target(seq, name, parent_taxid=1000, filename=filenames[f])
        dbb = b.finish(load=True)
        assert da.n_targets == dbb.n_targets == added and da.n_locations == dbb.n_locations > 0
        ka, sa = da.table_features()
        kb, sb = dbb.table_features()
        assert np.array_equal(ka, kb) and np.array_equal(sa, sb) and len(ka) > 0
        oa, la = da.table_lookup(ka)
        ob, lb = dbb.table_lookup(kb)
        assert np.array_equal(oa, ob) and np.array_equal(la, lb)
        assert [target_windows(a, t) for t in range(added)] == [target_windows(b, t) for t in range(added)]
    finally:
        for d in (da, dbb):
            if d is not None:
                d.close()
        a.free()
        b.free()
