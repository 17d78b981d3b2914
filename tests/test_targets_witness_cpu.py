"""CPU: the target rule in plain Python (targets_ref, the model of mc_parse_targets) against the record rule (parse_ref) on every case of
targets_cases: file by file, and on the files joined with a '\\n' put where one lacks it -- the claim that the per-file rule IS the record
rule.  The irregular cases and the bad tables get the model's verdict, offence and file.  And the argument checks of mc_parse_targets that
need no device, on an mc_open_metadata context."""
import ctypes as C
import os

import numpy as np

import parse_cases
import parse_ref
import targets_cases
import targets_ref
from metacache_amd import api

GOLDEN = parse_cases.GOLDEN


def test_case_lists_are_complete():
    T = api.parse_tile()
    assert sorted(targets_cases.regular_cases(T)) == targets_cases.REGULAR_NAMES
    assert sorted(targets_cases.irregular_cases(T)) == targets_cases.IRREGULAR_NAMES
    assert sorted(targets_cases.bad_tables()) == targets_cases.BAD_TABLE_NAMES


def test_cases_lie_where_they_are_meant_to():
    T = api.parse_tile()
    cases = targets_cases.regular_cases(T)
    for d in (-1, 0, 1):
        assert int(targets_ref.table_of(cases[f"file_start_at_T{d:+d}"])[1]) == T + d
    for d in (-1, 0):
        files = cases[f"no_final_newline_end_at_T{d:+d}"]
        assert len(files[0]) == T + d and not files[0].endswith(b"\n")
    off = targets_ref.table_of(cases["tiny_files"])
    assert max(sum(1 for o in off[:-1] if g <= int(o) < g + 16) for g in range(0, int(off[-1]), 16)) >= 8       # file starts in one thread's bytes
    assert all(len(f) == 1 for f in cases["tiny_files_only"])
    long_one = targets_ref.parse(cases["long_record"]).records[1]
    assert len(long_one[2]) > 2 * T
    assert int(targets_ref.table_of(cases["many_tiles"])[-1]) > parse_cases.SCAN_TRIP * T
    hdr_off, hdr_len = targets_ref.parse(cases["header_across"]).records[-2][:2]
    assert hdr_off < T < hdr_off + hdr_len
    assert len(cases["golden_genomes"]) == 3


def test_seq_may_need_more_bytes_than_the_range_holds():
    """the bound the staging buffers are sized by: nbytes + files + 16, reached by files that end in a record of len % 4 == 1"""
    cases = targets_cases.regular_cases(api.parse_tile())
    for name, files in cases.items():
        need = int(targets_ref.pack(targets_ref.parse(files))["status"][2])
        assert need <= sum(len(f) for f in files) + len(files) + 16, name
    for name in ("tight_tail_1", "tight_tail_5", "tight_tails_in_a_row"):
        files = cases[name]
        assert int(targets_ref.pack(targets_ref.parse(files))["status"][2]) == sum(len(f) for f in files) + len(files) + 16, name


def test_buffer_calls_check_their_arguments_without_a_device():
    L = api.lib()
    L.mc_buffer_alloc.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_void_p)]
    L.mc_buffer_free.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.mc_buffer_free.restype = None
    h, out = C.c_void_p(), C.c_void_p(1)
    assert L.mc_open_metadata(os.path.join(GOLDEN, "toy32").encode(), C.byref(h)) == api.MC_OK
    try:
        assert L.mc_buffer_alloc(None, 64, 0, C.byref(out)) == -1
        assert L.mc_buffer_alloc(h, 64, 0, None) == -1 and L.mc_buffer_alloc(h, 0, 0, C.byref(out)) == -1
        assert L.mc_buffer_alloc(h, 64, 2, C.byref(out)) == -1 and L.mc_buffer_alloc(h, 64, -1, C.byref(out)) == -1
        assert L.mc_buffer_alloc(h, 64, 0, C.byref(out)) == -6 and out.value is None and b"no device" in L.mc_last_error(h)
        assert L.mc_buffer_alloc(h, 64, 1, C.byref(out)) == -6
        buf = np.zeros(8, dtype=np.uint64)
        L.mc_buffer_free(None, buf.ctypes.data, 0); L.mc_buffer_free(h, None, 0); L.mc_buffer_free(h, buf.ctypes.data, 2)
        L.mc_buffer_free(h, buf.ctypes.data, 0); L.mc_buffer_free(h, buf.ctypes.data, 1)      # (a context without a device owns no such memory: nothing happens)
    finally:
        L.mc_destroy(h)


def test_model_equals_the_record_rule_file_by_file():
    for name, files in targets_cases.regular_cases(api.parse_tile()).items():
        data, off = b"".join(files), targets_ref.table_of(files)
        got = targets_ref.parse(files)
        assert got.verdict == targets_ref.OK, (name, got.offence)
        k = 0
        for f, one in enumerate(files):
            alone = parse_ref.parse(one)
            assert alone.verdict == parse_ref.OK, (name, f)
            for i, (h, hl, seq) in enumerate(alone.records):
                assert got.records[k] == (int(off[f]) + h, hl, seq, f, i), (name, f, i)
                assert data[got.records[k][0]:got.records[k][0] + hl] == one[h:h + hl]
                k += 1
        assert k == len(got.records), name


def test_per_file_rule_is_the_record_rule_on_the_joined_files():
    for name, files in targets_cases.regular_cases(api.parse_tile()).items():
        joined = b"".join(f if f.endswith(b"\n") else f + b"\n" for f in files)
        whole = parse_ref.parse(joined)
        got = targets_ref.parse(files)
        assert whole.verdict == parse_ref.OK, name
        data = b"".join(files)
        assert [(joined[h:h + hl], s) for h, hl, s in whole.records] == [(data[r[0]:r[0] + r[1]], r[2]) for r in got.records], name


def test_model_on_irregular_ranges_and_bad_tables():
    for name, (files, f, at) in targets_cases.irregular_cases(api.parse_tile()).items():
        got = targets_ref.parse(files)
        assert (got.verdict, got.offence, got.file) == (targets_ref.IRREGULAR, int(targets_ref.table_of(files)[f]) + at, f), name
        assert targets_ref.pack(got)["status"].tolist() == [0, 0, 0, 0, 1, got.offence, 0, f], name
    for name, (data, off, row) in targets_cases.bad_tables().items():
        got = targets_ref.parse_range(data, off)
        assert (got.verdict, got.offence, got.file) == (targets_ref.IRREGULAR, len(data), row), name


def test_model_details():
    files = [b">a b\r\nAC\r\n\r\nGTA\r\n>c\r\n", b">", b">d\nT"]
    p = targets_ref.parse(files)
    assert p.records == [(1, 3, b"ACGTA", 0, 0), (18, 1, b"", 0, 1), (22, 0, b"", 1, 0), (23, 1, b"T", 2, 0)]
    w = targets_ref.pack(p)
    assert w["targets"].tolist() == [(0, 5, 0, 0, 0), (8, 0, 0, 1, 0), (8, 0, 1, 0, 0), (8, 1, 2, 0, 0)]
    assert w["seq"] == b"ACGTA\0\0\0T\0\0\0" + b"\0" * 16 and w["status"].tolist() == [4, 2, 28, 0, 0, 0, 5, 0]
    assert targets_ref.headers_of(b"".join(files), p) == [b"a b", b"c", b"", b"d"]


def test_argument_checks_need_no_device():
    L = api.lib()
    h = C.c_void_p()
    assert L.mc_open_metadata(os.path.join(GOLDEN, "toy32").encode(), C.byref(h)) == api.MC_OK
    try:
        data = np.frombuffer(b">a\nACGT\n" + b"\0" * 56, dtype=np.uint8).copy()
        table = np.array([0, 8], dtype=np.uint64)
        buf = np.zeros(4096, dtype=np.uint64)                       # (8-byte aligned; its address is only compared, never read: no device)
        base = buf.ctypes.data + (-buf.ctypes.data) % 16
        status = np.zeros(8, dtype=np.uint64)

        def call(bytes_ptr=data.ctypes.data, nbytes=8, file_off=table.ctypes.data, num_files=1, flags=api.PARSE_HOST, status_ptr=status.ctypes.data, hdr=base,
                 targets=base + 64, seq=base + 256, seq_cap=64, ws=None, ws_bytes=0, max_records=2, out=True):
            o = api.McParseTargetsOutput(hdr, targets, seq, seq_cap, status_ptr, max_records)
            return L.mc_parse_targets(h, bytes_ptr, nbytes, file_off, num_files, flags, C.byref(o) if out else None, ws, ws_bytes, None)

        assert L.mc_parse_targets(None, data.ctypes.data, 8, table.ctypes.data, 1, api.PARSE_HOST, None, None, 0, None) == -1
        assert call(out=False) == -1
        assert call(flags=api.PARSE_HOST | 2) == -1 and call(flags=4) == -1
        assert call(bytes_ptr=None) == -1 and call(nbytes=0) == -1 and call(nbytes=(1 << 31) + 1) == -1
        assert call(file_off=None) == -1 and call(num_files=0) == -1
        assert call(status_ptr=None) == -1
        assert call(hdr=None) == -1 and call(targets=None) == -1
        assert call(seq=None) == -1
        # MC_PARSE_HOST: the table is read on the host
        for bad in ([1, 8], [0, 7], [0, 9]):
            t = np.array(bad, dtype=np.uint64)
            assert call(file_off=t.ctypes.data) == -1
            assert b"file table" in L.mc_last_error(h)
        t3 = np.array([0, 4, 4, 8], dtype=np.uint64)
        assert call(file_off=t3.ctypes.data, num_files=3) == -1
        # the device form: workspace and alignment, checked before any device call
        need = api.parse_targets_scratch_bytes(8, 1, 2)
        assert need >= 256 and api.parse_targets_scratch_bytes(1 << 31, 1, 2) > api.parse_targets_scratch_bytes(1 << 30, 1, 2) > need
        assert api.parse_targets_scratch_bytes(8, 1 << 20, 2) > need and api.parse_targets_scratch_bytes(8, 1, 1 << 20) > need
        dev = dict(flags=0, bytes_ptr=base + 3072, file_off=base + 3200, ws=base + 4096, ws_bytes=need)
        assert call(**{**dev, "ws": None}) == -1 and call(**{**dev, "ws_bytes": need - 1}) == -1
        assert call(**{**dev, "bytes_ptr": base + 3073}) == -1 and call(**{**dev, "seq": base + 260}) == -1 and call(**{**dev, "ws": base + 4100}) == -1
        assert call(**{**dev, "status_ptr": status.ctypes.data + 4}) == -1 and call(**{**dev, "targets": base + 68}) == -1
        assert call(**{**dev, "file_off": base + 3204}) == -1 and call(**{**dev, "hdr": base + 2}) == -1
        # arguments in order: the context has no device
        assert call(**dev) == -6 and call() == -6
        assert b"no device" in L.mc_last_error(h)
        assert not status.any()
        st = np.ones(4, dtype=np.uint64)
        assert L.mc_parse_stats(h, st.ctypes.data) == 0 and not st.any()
    finally:
        L.mc_destroy(h)
