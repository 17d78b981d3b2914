"""CPU: the cut rule of mc_parse_cut in plain Python (cut_ref) is held to the record rule (parse_ref), which test_parse_witness_cpu holds
to the host reader: every batch of a cut is a range of whole records, the batches together are the records in front of `consumed`, a
refused range is refused where the record rule refuses it, and open cuts chained piece by piece give the file's records in order.
Also: mc_parse_cut / mc_parse_headers / the device-byte slot look at their arguments before any device call and fail loudly without one."""
import ctypes as C
import os

import numpy as np
import pytest

import cut_cases
import cut_ref
import parse_cases
import parse_ref
from metacache_amd import api

GOLDEN = parse_cases.GOLDEN
T = 4096                                                            # (the cases are built around a tile; the model does not care which)
CASES = cut_cases.all_cases(T)
PARSED = {}


def parsed_prefix(name, data, consumed):
    key = (name, consumed)
    if key not in PARSED:
        PARSED[key] = parse_ref.parse(data[:consumed])
    return PARSED[key]


def batch_sizes(whole, pairs):
    rs = {1, 2, 3, 23, max(whole, 1), whole + 1}
    return sorted({r + (r & 1) for r in rs} if pairs else rs)


def records_of_slices(data, cuts):
    out = []
    for a, b in zip(cuts, cuts[1:]):
        p = parse_ref.parse(data[a:b])
        assert p.verdict == parse_ref.OK, (a, b, p.offence)
        out.append([(a + h, l, s) for h, l, s in p.records])
    return out


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("open_end", [False, True])
def test_every_batch_is_a_range_of_whole_records(name, open_end):
    data, pairs = CASES[name]
    whole = cut_ref.cut(data, 2, pairs, open_end).whole
    for R in batch_sizes(whole, pairs):
        c = cut_ref.cut(data, R, pairs, open_end)
        assert c.consumed <= len(data) and c.whole == whole and (open_end or c.consumed == len(data))
        if c.consumed == 0:
            assert data[0:1] not in (b">", b"@") or (c.verdict == parse_ref.OK and c.cuts == [0] and c.whole == 0)
            continue
        want = parsed_prefix(name, data, c.consumed)
        if c.verdict != parse_ref.OK:
            assert (c.verdict, c.offence) == (want.verdict, want.offence), (name, R)
            assert c.cuts == []
            continue
        assert want.verdict == parse_ref.OK and len(want.records) == c.whole, (name, R)
        assert c.cuts[0] == 0 and c.cuts[-1] == c.consumed and len(c.cuts) == -(-c.whole // R) + 1
        per = records_of_slices(data, c.cuts)
        assert [len(b) for b in per] == [min(R, c.whole - k) for k in range(0, c.whole, R)], (name, R)
        assert [r for b in per for r in b] == want.records, (name, R)
        assert c.longest == max(b - a for a, b in zip(c.cuts, c.cuts[1:]))
        assert c.half == (1 if (not open_end and pairs and c.whole & 1) else 0)


def small_file(fastq, nl):
    rng = np.random.default_rng(3)
    rec = parse_cases.fastq_record if fastq else (lambda n, s: parse_cases.fasta_record(n, s, 25))
    d = b"".join(rec(b"r%d some words" % i, parse_cases.dna(rng, 40 + 7 * i)) for i in range(5 if fastq else 7))
    return parse_cases.crlf(d) if nl == 2 else d


@pytest.mark.parametrize("fastq", [False, True])
@pytest.mark.parametrize("nl", [1, 2])
@pytest.mark.parametrize("pairs", [False, True])
def test_every_prefix_through_the_open_rule(fastq, nl, pairs):
    data = small_file(fastq, nl)
    assert 500 < len(data) < 900
    whole_seen = set()
    for p in range(1, len(data) + 1):
        c = cut_ref.cut(data[:p], 2, pairs, True)
        assert c.consumed <= p
        if c.consumed == 0:
            assert c.verdict == parse_ref.OK and c.whole == 0
            continue
        want = parse_ref.parse(data[:c.consumed])
        assert (c.verdict, c.offence if c.verdict else 0) == (want.verdict, want.offence if want.verdict else 0), p
        assert c.verdict == parse_ref.OK and len(want.records) == c.whole      # (a regular file: every prefix of whole records is regular)
        whole_seen.add(c.whole)
    assert max(whole_seen) >= 4 and len(whole_seen) >= 2


def chain(data, R, pairs, sizes):
    """open cuts piece by piece, one closed cut of the rest -> the records of every batch, in order"""
    n, pos, k, out = len(data), 0, 0, []
    while pos < n:
        size = sizes[k % len(sizes)]
        k += 1
        while True:
            last = pos + size >= n
            c = cut_ref.cut(data[pos:pos + size], R, pairs, open=not last)
            if last or c.consumed:
                break
            size *= 2                                                     # no whole record in the piece: a larger piece
        assert c.verdict == parse_ref.OK, (pos, size, c.offence)
        for b in records_of_slices(data, [pos + x for x in c.cuts]):
            out += b
        pos += c.consumed
    return out


@pytest.mark.parametrize("name", parse_cases.REGULAR)
@pytest.mark.parametrize("nl", [1, 2])
def test_chained_pieces_give_the_records_of_the_file(name, nl):
    data = parse_cases.golden_bytes(name)
    if nl == 2:
        data = parse_cases.crlf(data)
    want = parse_ref.parse(data)
    assert want.verdict == parse_ref.OK
    rng = np.random.default_rng(len(data))
    for pairs, R in ((False, 3), (True, 4)):
        if pairs and len(want.records) & 1:
            continue
        sizes = [int(x) for x in rng.integers(60, 3000, 16)]
        assert chain(data, R, pairs, sizes) == want.records, (name, pairs)


def test_model_details():
    assert cut_ref.cut(b">a\nAC\n>b\nGT\n", 1, open=True)[:5] == (0, 0, 1, 6, [0, 6])
    assert cut_ref.cut(b">a\nAC\n", 1, open=True)[:5] == (0, 0, 0, 0, [0])
    assert cut_ref.cut(b"@a\nAC\n+\nII\n@b\nA", 1, open=True)[:5] == (0, 0, 1, 11, [0, 11])
    assert cut_ref.cut(b"@a\nAC\n+\nII\n@b\nA", 1)[:2] == (parse_ref.IRREGULAR, 15)
    assert cut_ref.cut(b"@a\nAC\n+\nII", 1, open=True)[:5] == (0, 0, 0, 0, [0])
    assert cut_ref.cut(b"ACGT\n>a\nAC\n", 1)[:2] == cut_ref.cut(b"ACGT\n>a\nAC\n", 1, open=True)[:2] == (parse_ref.IRREGULAR, 0)
    assert cut_ref.cut(b">a\n+\n>b\nAC\n>c\n", 1, open=True)[:2] == (parse_ref.IRREGULAR, 3)
    assert cut_ref.cut(b">a\nAC\n>b\n+\n", 1, open=True)[:4] == (0, 0, 1, 6)          # the offence lies behind consumed
    assert cut_ref.cut(b">a\nAC\n>b\nGT\n>c\nA\n", 2, pairs=True)[4:] == ([0, 12, 17], 3, 12, 1)
    assert cut_ref.cut(b">a\nAC\n>b\nGT\n>c\nA\n", 2, pairs=True, open=True)[2:5] == (2, 12, [0, 12])
    assert cut_ref.headers(b">a b\r\nAC\n>\nGT\n", parse_ref.parse(b">a b\r\nAC\n>\nGT\n")) == (b"a b", [0, 3, 3])


def test_argument_checks_need_no_device():
    L = api.lib()
    h = C.c_void_p()
    assert L.mc_open_metadata(os.path.join(GOLDEN, "toy32").encode(), C.byref(h)) == api.MC_OK
    try:
        data = np.frombuffer(b">a\nACGT\n" + b"\0" * 56, dtype=np.uint8).copy()
        buf = np.zeros(4096, dtype=np.uint64)                       # (its address is only compared, never read: no device)
        base = buf.ctypes.data + (-buf.ctypes.data) % 16
        status = np.zeros(8, dtype=np.uint64)
        need = api.parse_cut_scratch_bytes(8)
        assert need >= 256 and api.parse_cut_scratch_bytes(1 << 31) > api.parse_cut_scratch_bytes(1 << 30) > need

        def cut(ctx=h, bytes_ptr=data.ctypes.data, nbytes=8, R=2, flags=api.PARSE_HOST, cuts=base, capacity=4, status_ptr=status.ctypes.data, ws=None, ws_bytes=0):
            return L.mc_parse_cut(ctx, bytes_ptr, nbytes, R, flags, cuts, capacity, status_ptr, ws, ws_bytes, None)

        assert cut(ctx=None) == -1
        assert cut(flags=api.PARSE_HOST | 8) == -1
        assert cut(bytes_ptr=None) == -1 and cut(nbytes=0) == -1 and cut(nbytes=(1 << 31) + 1) == -1
        assert cut(R=0) == -1 and cut(R=3, flags=api.PARSE_HOST | api.PARSE_PAIRS) == -1
        assert b"odd" in L.mc_last_error(h)
        assert cut(cuts=None) == -1 and cut(status_ptr=None) == -1
        dev = dict(flags=api.CUT_OPEN, bytes_ptr=base + 3073, ws=base + 4096, ws_bytes=need)           # (bytes at any address)
        assert cut(**{**dev, "ws": None}) == -1 and cut(**{**dev, "ws_bytes": need - 1}) == -1
        assert cut(**{**dev, "ws": base + 4100}) == -1 and cut(**{**dev, "cuts": base + 4}) == -1 and cut(**{**dev, "status_ptr": status.ctypes.data + 4}) == -1
        assert cut(**dev) == -6 and cut() == -6                      # arguments in order: the context has no device
        assert b"no device" in L.mc_last_error(h)

        hneed = api.parse_headers_scratch_bytes(4)
        assert hneed >= 256 and api.parse_headers_scratch_bytes(1 << 24) > hneed

        def heads(ctx=h, bytes_ptr=data.ctypes.data, nbytes=8, hdr=base, ps=base + 64, mr=4, flags=api.PARSE_HOST, out=base + 256, cap=64, off=base + 512,
                  status_ptr=status.ctypes.data, ws=None, ws_bytes=0):
            return L.mc_parse_headers(ctx, bytes_ptr, nbytes, hdr, ps, mr, flags, out, cap, off, status_ptr, ws, ws_bytes, None)

        assert heads(ctx=None) == -1 and heads(flags=api.PARSE_HOST | api.PARSE_PAIRS) == -1
        assert heads(bytes_ptr=None) == -1 and heads(nbytes=0) == -1 and heads(nbytes=(1 << 31) + 1) == -1
        assert heads(ps=None) == -1 and heads(status_ptr=None) == -1 and heads(off=None) == -1 and heads(hdr=None) == -1 and heads(out=None) == -1
        dev = dict(flags=0, bytes_ptr=base + 3073, out=base + 257, ws=base + 4096, ws_bytes=hneed)
        assert heads(**{**dev, "ws": None}) == -1 and heads(**{**dev, "ws_bytes": hneed - 1}) == -1 and heads(**{**dev, "ws": base + 4100}) == -1
        assert heads(**{**dev, "ps": base + 68}) == -1 and heads(**{**dev, "off": base + 516}) == -1 and heads(**{**dev, "hdr": base + 2}) == -1
        assert heads(**dev) == -6 and heads() == -6
        assert b"no device" in L.mc_last_error(h)
        assert not status.any()
        # the slot calls: a context without a device has no slots, and every argument is looked at before anything else
        text, off, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        assert L.mc_batch_add_device_bytes(None, 0, base, 8, 0, 0) == -1 and L.mc_batch_add_device_bytes(h, 0, base, 8, 0, 0) == -1
        assert L.mc_batch_headers(None, 0, C.byref(text), C.byref(off), C.byref(n)) == -1 and L.mc_batch_headers(h, 0, C.byref(text), C.byref(off), C.byref(n)) == -1
        # a resident file: the same order
        inp, info = C.c_void_p(), np.ones(8, dtype=np.uint64)
        op = lambda ctx=h, b=data.ctypes.data, n=8, flags=0, R=2, piece=1 << 20, slot=1 << 20, out=C.byref(inp), inf=info.ctypes.data: L.mc_input_open(ctx, b, n, flags, R, piece, slot, 1 << 40, out, inf)
        assert op(ctx=None) == -1 and op(out=None) == -1 and op(inf=None) == -1 and op(b=None) == -1 and op(n=0) == -1 and op(flags=4) == -1
        assert op(R=0) == -1 and op(R=3, flags=api.PARSE_PAIRS) == -1 and op(piece=0) == -1 and op(piece=(1 << 31) + 1) == -1 and op(slot=0) == -1
        assert op() == -6 and b"no device" in L.mc_last_error(h) and not inp.value
        assert L.mc_input_batches(None, None, 0, None, None) == -1 and L.mc_input_download(None, None, 0) == -1
        L.mc_input_close(None)                                      # a no-op
    finally:
        L.mc_destroy(h)
