"""CPU: the record rule in plain Python (parse_ref, the model of mc_parse_records) against SeqFile's eager index (mcq_common.h), record by
record -- header and sequence -- on the seven golden read files and on the generated edge files of parse_cases; the irregular files must
get the irregular verdict from the model and the exact reader from SeqFile.  SeqFile itself is held to the reference's reader by the
command line's golden outputs (test_cli_gpu.py, cli_expected.json.gz), so the model stands on the same ground.
And the argument checks of mc_parse_records, mc_batch_add_file_bytes and mc_batch_records that need no device, on an mc_open_metadata context."""
import ctypes as C
import os
import subprocess

import numpy as np

import parse_cases
import parse_ref
from metacache_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = parse_cases.GOLDEN


def dump_records(tmp_path, paths):
    exe = str(tmp_path / "seqfile_records_dump")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "metacache_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "seqfile_records_dump.cpp"), "-o", exe, "-lz", "-pthread"])
    r = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out, lines, k = [], r.stdout.split("\n"), 0
    for _ in paths:
        _, n, how, b, e = lines[k].split(" ")
        recs = []
        for line in lines[k + 1:k + 1 + int(n)]:
            h, s = line.split(" ")
            recs.append((bytes.fromhex(h), bytes.fromhex(s)))
        out.append((how, int(b), int(e), recs))
        k += 1 + int(n)
    return out


def test_model_equals_seqfile_on_every_record(tmp_path):
    cases = parse_cases.all_cases(api.parse_tile())
    assert sorted(cases) == sorted(parse_cases.CASE_NAMES)
    for name in parse_cases.IRREGULAR:
        cases[name] = parse_cases.golden_bytes(name)
    names = sorted(cases)
    paths = []
    for k, name in enumerate(names):
        paths.append(str(tmp_path / f"case{k}.txt"))
        with open(paths[-1], "wb") as f:
            f.write(cases[name])
    for name, (how, b, e, recs) in zip(names, dump_records(tmp_path, paths)):
        data = cases[name]
        parsed = parse_ref.parse(data)
        if name in parse_cases.IRREGULAR:
            assert parsed.verdict == parse_ref.IRREGULAR and how == "exact", name
            continue
        assert parsed.verdict == parse_ref.OK and how == "fast" and (b, e) == (0, len(data)), (name, how, parsed.offence)
        assert len(recs) == len(parsed.records), name
        for i, ((h, s), (ho, hl, seq)) in enumerate(zip(recs, parsed.records)):
            assert h == data[ho:ho + hl] and s == seq, (name, i)


def test_the_offence_of_the_golden_irregular_files():
    """cli_irregular.fa: the first of its ten '+' lines; cli_irregular.fq: the second sequence line of its first record"""
    fa = parse_cases.golden_bytes("cli_irregular.fa")
    p = parse_ref.parse(fa)
    assert p.verdict == parse_ref.IRREGULAR and fa[p.offence:p.offence + 1] == b"+" and fa[p.offence - 1:p.offence] == b"\n"
    assert sum(1 for b, _ in parse_ref.lines_of(fa) if fa[b:b + 1] == b"+") == 10 and b"\n+" not in fa[:p.offence]
    fq = parse_cases.golden_bytes("cli_irregular.fq")
    p = parse_ref.parse(fq)
    assert p.verdict == parse_ref.IRREGULAR and p.offence == parse_ref.lines_of(fq)[2][0]


def test_model_details():
    p = parse_ref.parse(b">a b\r\nAC\r\n\r\nGT\r\n>c\r\n")
    assert p.records == [(1, 3, b"ACGT"), (17, 1, b"")]
    assert parse_ref.name_of(b">a b\r\n", 1, 3) == b"a"
    w = parse_ref.pack(b">a b\r\nAC\r\n\r\nGT\r\n>c\r\n", p, pairs=True, insert_max=0, stride=2)
    assert w["qinfo"].tolist() == [[0, 4, 4, 0]] and w["names"] == b"a" and w["max_win"].tolist() == [4] and w["status"].tolist() == [2, 1, 20, 1, 0, 0, 4, 0]
    w = parse_ref.pack(b"@x\nACGTA\n+\nIIIII\n", parse_ref.parse(b"@x\nACGTA\n+\nIIIII\n"), pairs=True)
    assert w["qinfo"].tolist() == [[0, 5, 8, 0]] and w["seq"] == b"ACGTA\0\0\0" + b"\0" * 16 and int(w["status"][7]) == 1
    assert parse_ref.parse(b"@x\nAC\nGT\n+\nIIII\n")[:2] == (parse_ref.IRREGULAR, 6)
    assert parse_ref.parse(b"@x\nAC\n+\n")[:2] == (parse_ref.IRREGULAR, 8)


def test_argument_checks_need_no_device():
    L = api.lib()
    h = C.c_void_p()
    assert L.mc_open_metadata(os.path.join(GOLDEN, "toy32").encode(), C.byref(h)) == api.MC_OK
    try:
        data = np.frombuffer(b">a\nACGT\n" + b"\0" * 56, dtype=np.uint8).copy()
        buf = np.zeros(4096, dtype=np.uint64)                       # (8-byte aligned; its address is only compared, never read: no device)
        base = buf.ctypes.data + (-buf.ctypes.data) % 16
        status = np.zeros(8, dtype=np.uint64)

        def call(bytes_ptr=data.ctypes.data, nbytes=8, flags=api.PARSE_HOST, status_ptr=status.ctypes.data, hdr=base, seq=base + 256, seq_cap=64,
                 names_cap=64, ws=None, ws_bytes=0, max_records=4, out=True):
            o = api.McParseOutput(hdr, base + 64, seq, seq_cap, base + 512, names_cap, base + 1024, base + 2048, status_ptr, max_records)
            return L.mc_parse_records(h, bytes_ptr, nbytes, flags, 0, C.byref(o) if out else None, ws, ws_bytes, None)

        assert L.mc_parse_records(None, data.ctypes.data, 8, api.PARSE_HOST, 0, None, None, 0, None) == -1
        assert call(out=False) == -1
        assert call(flags=api.PARSE_HOST | 4) == -1
        assert call(bytes_ptr=None) == -1 and call(nbytes=0) == -1
        assert call(nbytes=(1 << 31) + 1) == -1
        assert call(status_ptr=None) == -1
        assert call(hdr=None) == -1
        assert call(seq=None) == -1 and call(seq_cap=1 << 32) == -1 and call(names_cap=1 << 32) == -1
        wrong = np.frombuffer(b"ACGT\n>a\n", dtype=np.uint8).copy()
        assert call(bytes_ptr=wrong.ctypes.data) == -1            # MC_PARSE_HOST: bytes[0] is read on the host
        assert b"'>' or '@'" in L.mc_last_error(h)
        # the device form: workspace and alignment, checked before any device call
        need = api.parse_scratch_bytes(8)
        assert need >= 256 and api.parse_scratch_bytes(1 << 31) > api.parse_scratch_bytes(1 << 30) > need
        dev = dict(flags=0, bytes_ptr=base + 3072, ws=base + 4096, ws_bytes=need)
        assert call(**{**dev, "ws": None}) == -1 and call(**{**dev, "ws_bytes": need - 1}) == -1
        assert call(**{**dev, "bytes_ptr": base + 3073}) == -1 and call(**{**dev, "seq": base + 260}) == -1 and call(**{**dev, "ws": base + 4100}) == -1
        assert call(**{**dev, "status_ptr": status.ctypes.data + 4}) == -1 and call(**{**dev, "hdr": base + 2}) == -1
        # arguments in order: the context has no device
        assert call(**dev) == -6 and call() == -6
        assert b"no device" in L.mc_last_error(h)
        assert not status.any()
        # the slot calls: a context without a device has no slots, and every argument is looked at before anything else
        info = api.McBatchRecordInfo()
        assert L.mc_batch_add_file_bytes(None, 0, data.ctypes.data, 8, 0, 0) == -1 and L.mc_batch_add_file_bytes(h, 0, data.ctypes.data, 8, 0, 0) == -1
        assert L.mc_batch_records(None, 0, C.byref(info)) == -1 and L.mc_batch_records(h, 0, C.byref(info)) == -1 and L.mc_batch_records(h, 0, None) == -1
        st = np.ones(4, dtype=np.uint64)
        assert L.mc_parse_stats(h, st.ctypes.data) == 0 and not st.any() and L.mc_parse_stats(h, None) == -1
    finally:
        L.mc_destroy(h)
