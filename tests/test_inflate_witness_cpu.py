"""CPU: the BGZF rule in plain Python (inflate_ref) against zlib on every generated case -- equal bytes, the same refusals plus the trailer
rules, and the features each case is named for; mc_bgzf_index (host code, no device) against the model's walk; and the argument checks of
mc_inflate_blocks that need no device, on an mc_open_metadata context."""
import ctypes as C
import gzip
import os
import random
import struct
import zlib

import numpy as np
import pytest

import inflate_cases as cases
import inflate_ref as ref
from metacache_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def zlib_raw(payload):
    """(bytes, bytes left behind the stream) as zlib reads a raw deflate stream, or None where it refuses"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(payload)
    except zlib.error:
        return None
    return (out, len(d.unused_data)) if d.eof else None


def test_model_equals_zlib_on_the_good_cases():
    feats = {}
    for name, (m, plain) in cases.good_cases().items():
        assert gzip.decompress(m) == plain, name
        out, left, feats[name] = ref.inflate_stream(ref.payload_of(m))
        assert (out, left) == zlib_raw(ref.payload_of(m)) == (plain, 0), name
        assert ref.inflate_member(m) == plain, name
        assert ref.walk(m) == ([(0, 0, len(m), len(plain))], len(plain), ref.BGZF_OK, 0), name
    # a case covers what it is named for
    assert feats["stored_level0"]["types"] == [0, 0] and feats["noise_stored"]["types"] == [0, 0] and len(cases.good_cases()["noise_stored"][0]) == 65316
    assert feats["fixed"]["types"] == [1] and feats["eof"]["types"] == [1] and len(cases.good_cases()["eof"][0]) == 28
    for name in ("dynamic_l1", "dynamic_l6", "dynamic_l9", "dynamic_rle", "dynamic_huffman_only"):
        assert set(feats[name]["types"]) == {2}, name
    assert feats["dynamic_huffman_only"]["longest_match"] == 0 and feats["dynamic_rle"]["max_dist"] == 1 and feats["dynamic_rle"]["overlaps"] > 0
    assert feats["two_blocks_flush"]["types"] == [2, 0, 2]
    assert feats["fibonacci_15bit"]["types"] == [2, 2] and feats["fibonacci_15bit"]["longest_code"] == 15
    f = feats["far_match"]
    assert (f["max_dist"], f["min_dist"], f["longest_match"]) == (32768, 1, 258) and f["overlaps"] >= 128
    assert len(cases.good_cases()["far_match"][1]) == 33292
    big = cases.good_cases()["largest_expansion"]
    assert len(big[0]) < 300 and len(big[1]) == 65536 and feats["largest_expansion"]["min_dist"] == 1 and feats["largest_expansion"]["longest_match"] == 258
    assert len(cases.good_cases()["largest_isize"][1]) == 65536


def test_model_refuses_what_zlib_refuses_and_the_trailer_rules():
    want = dict(block_type_3=ref.R_BTYPE, stored_len_nlen=ref.R_STORED, distance_beyond_output=ref.R_DISTANCE, symbol_286=ref.R_SYMBOL,
                distance_code_30=ref.R_DISTANCE, cut_in_half=ref.R_INPUT, oversubscribed_code_lengths=ref.R_LENGTHS, repeat_16_first=ref.R_LENGTHS,
                repeat_past_the_end=ref.R_LENGTHS, wrong_crc=ref.R_CRC, isize_one_too_large=ref.R_SHORT, isize_one_too_small=ref.R_OVER,
                spare_byte=ref.R_LEFT)
    assert sorted(want) == sorted(cases.bad_cases())
    for name, m in cases.bad_cases().items():
        assert ref.walk(m)[2] == ref.BGZF_OK, name                 # a member by the walk: only its inside is bad
        z = zlib_raw(ref.payload_of(m))
        assert (z is None) == (name in cases.ZLIB_REFUSES), name
        with pytest.raises(ref.Refused) as e:
            ref.inflate_member(m)
        assert e.value.reason == want[name], name
        if z is None:
            with pytest.raises(ref.Refused):
                ref.inflate_stream(ref.payload_of(m))
        else:
            out, left, _ = ref.inflate_stream(ref.payload_of(m))
            assert (out, left) == z and left == (name == "spare_byte")


def test_model_equals_zlib_on_damaged_streams():
    """one damaged byte in a small stream of every kind: the model accepts exactly where zlib does, with zlib's bytes"""
    rnd = random.Random(17)
    text = cases.fastq_text(1500, 23)
    pays = [ref.payload_of(cases.bgzf_block(text, lv, st)) for lv, st in ((6, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED), (6, zlib.Z_HUFFMAN_ONLY), (0, zlib.Z_DEFAULT_STRATEGY))]
    pays.append(ref.payload_of(cases.bgzf_block(cases.fibonacci_payload(nbytes=3000), 6, zlib.Z_HUFFMAN_ONLY)))
    accepted = refused = 0
    for pay in pays:
        for _ in range(60):
            at = rnd.randrange(min(len(pay), 120)) if rnd.random() < 0.7 else rnd.randrange(len(pay))
            bad = bytearray(pay)
            bad[at] ^= 1 << rnd.randrange(8)
            z = zlib_raw(bytes(bad))
            try:
                out, left, _ = ref.inflate_stream(bytes(bad))
                assert z == (out, left)
                accepted += 1
            except ref.Refused:
                assert z is None
                refused += 1
    assert accepted > 20 and refused > 20


def index_of(data, capacity=None):
    blocks, out_bytes, verdict, offence = api.bgzf_index(data, capacity)
    return [tuple(int(x) for x in b) for b in blocks], out_bytes, verdict, offence


def test_bgzf_index_equals_the_walk():
    good = cases.good_cases()
    names = sorted(good)
    rnd = random.Random(2)
    for k in range(4):
        order = names[:] if k == 0 else rnd.sample(names, len(names))
        data = b"".join(good[n][0] for n in order if n != "eof") + (cases.EOF_BLOCK if k % 2 == 0 else b"")
        got = index_of(data)
        assert got == ref.walk(data) and got[2] == ref.BGZF_OK and got[1] == sum(len(good[n][1]) for n in order)
        assert gzip.decompress(data) == b"".join(good[n][1] for n in order if n != "eof")
    three = good["short_text"][0] + good["one_byte"][0] + cases.EOF_BLOCK
    assert index_of(three) == ref.walk(three) and len(index_of(three)[0]) == 3
    # capacity one short: info complete, the rows a prefix
    full = index_of(three)
    assert index_of(three, 2) == (full[0][:2],) + full[1:] and index_of(three, 0) == ([],) + full[1:]
    at = len(good["short_text"][0])

    def foreign(data, offence, members):
        got = index_of(data)
        assert got == ref.walk(data) and got[2:] == (ref.BGZF_FOREIGN, offence) and len(got[0]) == members, got[2:]

    with open(os.path.join(GOLDEN, "cli_reads.fa.gz"), "rb") as f:
        foreign(f.read(), 0, 0)
    foreign(b"", 0, 0)
    m = good["one_byte"][0]
    flg = bytearray(m); flg[3] = 0x0c
    foreign(good["short_text"][0] + bytes(flg), at, 1)
    no_bc = m[:12] + b"XX" + m[14:]
    foreign(good["short_text"][0] + no_bc, at, 1)
    _, plain = good["one_byte"]
    raw = ref.payload_of(m)
    twice = cases.member(raw, plain, extra=b"BC\x02\x00\x00\x00")
    foreign(twice, 0, 0)
    assert index_of(good["bc_behind_another_subfield"][0])[2] == ref.BGZF_OK
    untiled = bytearray(cases.member(raw, plain, extra=b"XY\x03\x00abc")); untiled[14] = 4        # XY now swallows a byte of BC: the rest does not tile
    foreign(bytes(untiled), 0, 0)
    short_tail = bytearray(cases.member(raw, plain, extra=b"XY\x01\x00a")); struct.pack_into("<H", short_tail, 10, 12)   # XLEN one past the subfields
    foreign(bytes(short_tail), 0, 0)
    foreign(three[:-1], len(three) - 28, 2)                                  # the last member ends beyond nbytes
    foreign(three[:at + 5], at, 1)
    foreign(three + b"\x00", len(three), 3)                                  # trailing bytes
    foreign(three + three[:11], len(three), 3)
    big = bytearray(m); struct.pack_into("<I", big, len(big) - 4, 65537)
    foreign(good["short_text"][0] + bytes(big), at, 1)
    ok = bytearray(m); struct.pack_into("<I", ok, len(ok) - 4, 65536)
    assert index_of(bytes(ok))[:3] == ([(0, 0, len(m), 65536)], 65536, ref.BGZF_OK)
    L = api.lib()
    info = np.zeros(4, dtype=np.uint64)
    assert L.mc_bgzf_index(None, 0, None, 0, None) == -1 and L.mc_bgzf_index(None, 5, None, 0, info.ctypes.data) == -1


def test_names_exported_and_declared():
    with open(os.path.join(ROOT, "include", "metacache_amd.h")) as f:
        header = f.read()
    for name in ("mc_bgzf_index", "mc_inflate_blocks", "mc_inflate_stats"):
        assert name in api.EXPORTS and hasattr(api.lib(), name) and ("int " + name + "(") in header
    for k, v in dict(MC_BGZF_FOREIGN=api.BGZF_FOREIGN, MC_INFLATE_HOST=api.INFLATE_HOST, MC_INFLATE_CORRUPT=api.INFLATE_CORRUPT, MC_INFLATE_OVERFLOW=api.INFLATE_OVERFLOW,
                     MC_INFLATE_R_BTYPE=ref.R_BTYPE, MC_INFLATE_R_STORED=ref.R_STORED, MC_INFLATE_R_LENGTHS=ref.R_LENGTHS, MC_INFLATE_R_SYMBOL=ref.R_SYMBOL,
                     MC_INFLATE_R_DISTANCE=ref.R_DISTANCE, MC_INFLATE_R_INPUT=ref.R_INPUT, MC_INFLATE_R_OVER=ref.R_OVER, MC_INFLATE_R_SHORT=ref.R_SHORT,
                     MC_INFLATE_R_LEFT=ref.R_LEFT, MC_INFLATE_R_CRC=ref.R_CRC).items():
        assert any(line.split()[:3] == ["#define", k, str(v)] for line in header.split("\n")), k
    assert api.bgzf_block_dtype.itemsize == 24
    assert (api.INFLATE_R_BTYPE, api.INFLATE_R_CRC) == (ref.R_BTYPE, ref.R_CRC)
    with open(os.path.join(ROOT, "metacache_amd", "build.py")) as f:
        assert '"inflate.hip"' in f.read()


def test_argument_checks_need_no_device():
    L = api.lib()
    h = C.c_void_p()
    assert L.mc_open_metadata(os.path.join(GOLDEN, "toy32").encode(), C.byref(h)) == api.MC_OK
    try:
        m = cases.good_cases()["short_text"][0]
        data = np.frombuffer(m + b"\0" * 16, dtype=np.uint8).copy()
        rows = np.array([(0, 0, len(m), 1234)], dtype=api.bgzf_block_dtype)
        out = np.zeros(4096, dtype=np.uint8)
        status = np.zeros(4, dtype=np.uint64)
        buf = np.zeros(1 << 14, dtype=np.uint64)                    # (its addresses are only compared, never read: no device)
        base = buf.ctypes.data + (-buf.ctypes.data) % 16

        def call(ctx=h, bytes_ptr=data.ctypes.data, nbytes=len(m), blocks=rows.ctypes.data, n=1, flags=api.INFLATE_HOST, out_ptr=out.ctypes.data, cap=1234,
                 status_ptr=status.ctypes.data):
            return L.mc_inflate_blocks(ctx, bytes_ptr, nbytes, blocks, n, flags, out_ptr, cap, status_ptr, None)

        assert call(ctx=None) == -1
        assert call(bytes_ptr=None) == -1 and call(blocks=None) == -1 and call(status_ptr=None) == -1
        assert call(out_ptr=None) == -1
        assert call(flags=2) == -1 and call(flags=api.INFLATE_HOST | 4) == -1
        assert call(out_ptr=data.ctypes.data + 100, cap=50) == -1 and b"overlaps" in L.mc_last_error(h)
        # the rows of the host form are checked on the host
        def with_rows(r):
            a = np.array(r, dtype=api.bgzf_block_dtype)
            return call(blocks=a.ctypes.data, n=len(a))
        assert with_rows([(0, 0, len(m) + 1, 1234)]) == -1                   # beyond nbytes
        assert with_rows([(0, 0, len(m), 65537)]) == -1
        assert with_rows([(0, 0, 300, 10), (299, 10, 100, 10)]) == -1        # members overlap
        assert with_rows([(0, 10, 300, 10), (300, 19, 100, 10)]) == -1       # slices overlap
        assert with_rows([(300, 0, 100, 10), (0, 10, 300, 10)]) == -1        # decreasing
        assert b"rows" in L.mc_last_error(h)
        # the device form: alignment, before any device call
        dev = dict(flags=0, bytes_ptr=base, blocks=base + 4096, out_ptr=base + 8192, status_ptr=base + 16384)
        assert call(**{**dev, "bytes_ptr": base + 8}) == -1 and call(**{**dev, "out_ptr": base + 8200}) == -1
        assert call(**{**dev, "blocks": base + 4100}) == -1 and call(**{**dev, "status_ptr": base + 16388}) == -1
        assert b"aligned" in L.mc_last_error(h)
        # arguments in order: the context has no device
        assert call(**dev) == -6 and call() == -6 and call(n=0) == -6
        assert b"no device" in L.mc_last_error(h)
        assert not status.any() and not out.any()
        st = np.ones(4, dtype=np.uint64)
        assert L.mc_inflate_stats(h, st.ctypes.data) == 0 and not st.any() and L.mc_inflate_stats(h, None) == -1 and L.mc_inflate_stats(None, st.ctypes.data) == -1
        assert L.mc_set_tuning(h, b"inflate_stage_bytes", 1 << 20) == 0
    finally:
        L.mc_destroy(h)
