"""CPU: the stream rule in plain Python (gzip_ref) against zlib on every generated row -- zlib's bytes chained over the members on the
good rows, the named reason on the bad ones, nothing accepted that zlib refuses on damaged copies; mc_gzip_hint (host code, no device)
against the model's header walk on every row and on their prefixes; and the argument checks of mc_inflate_streams that need no device,
on an mc_open_metadata context."""
import ctypes as C
import os
import random
import zlib

import numpy as np
import pytest

import gzip_cases as cases
import gzip_ref as ref
from metacache_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def zlib_chain(row):
    """the bytes zlib.decompressobj(wbits=31) gives, chained over the members up to the row's end -> (bytes, members), or None where it
    refuses any of them or the row ends inside one"""
    out, members, rest = [], 0, bytes(row)
    while rest:
        d = zlib.decompressobj(wbits=31)
        try:
            out.append(d.decompress(rest))
        except zlib.error:
            return None
        if not d.eof:
            return None
        rest = d.unused_data
        members += 1
    return (b"".join(out), members) if members else None


def test_model_gives_zlibs_bytes_on_the_good_rows():
    feats = {}
    for name, (row, plain) in cases.good_cases().items():
        z = zlib_chain(row)
        assert z is not None and z[0] == plain, name
        assert ref.inflate_row(row, len(plain)) == z, name
        assert ref.inflate_row(row, len(plain) + 77) == z, name + ": more room than bytes"
        pay = ref.header_at(row, 0, True)
        feats[name] = ref.inflate_stream(row[pay:len(row) - 8], 1 << 31)[2]
    # a case covers what it is named for
    good = cases.good_cases()
    assert len(good["one_member_200000"][1]) == 200000 and len(good["one_mib"][1]) == 1 << 20
    f = feats["match_258_at_32768_across_65536"]
    assert (f["max_dist"], f["longest_match"]) == (32768, 258) and len(good["match_258_at_32768_across_65536"][1]) == 65536 - 100 + 258 + 3
    assert len(good["match_3_at_32768_across_65536"][1]) == 65535 + 3 + 3 and len(good["fill_at_1_across_65536"][1]) == 65536 - 129 + 258 + 3
    t = feats["full_flush_pieces"]["types"]
    assert len(t) > 40 and 0 in t and 2 in t and all(t[i] == 0 for i in range(1, len(t) - 1, 2))        # a stored block between the dynamic ones
    t = feats["stored_65535_in_a_row"]["types"]
    row = good["stored_65535_in_a_row"][0]
    assert set(t) == {0} and len(t) >= 4 and all(row[10 + k * 65540:15 + k * 65540] == b"\x00\xff\xff\x00\x00" for k in range(3))
    assert feats["one_mib"]["max_dist"] > 20000
    assert zlib_chain(good["chain_of_3"][0])[1] == 3 and zlib_chain(good["chain_empty_middle"][0])[1] == 3
    assert good["fname_zero_at_byte_63_of_a_round"][0][10 + 63] == 0 and good["fname_zero_in_the_next_round"][0][10 + 64] == 0


def test_model_refuses_the_bad_rows_with_the_named_reason():
    for name, (row, cap, reason) in cases.bad_cases().items():
        with pytest.raises(ref.Refused) as e:
            ref.inflate_row(row, cap)
        assert e.value.reason == reason, f"{name}: {e.value.reason}, named for {reason}"
    bad = cases.bad_cases()
    assert bad["wrong_crc_in_the_first_of_two"][0] and zlib_chain(bad["wrong_crc_in_the_first_of_two"][0]) is None
    # what the rule refuses beyond zlib: FHCRC; zlib reads that file
    assert zlib_chain(bad["fhcrc"][0]) is not None
    # the chain rule is what refuses the reach into the first member: as ONE history the match would be good
    with pytest.raises(ref.Refused) as e:
        ref.inflate_row(bad["second_member_reaches_into_the_first"][0], 1 << 20)
    assert (e.value.reason, e.value.members) == (ref.R_DISTANCE, 1)
    assert zlib_chain(bad["second_member_reaches_into_the_first"][0]) is None


def test_model_accepts_nothing_zlib_refuses_on_damaged_rows():
    """one damaged bit in a small row of every kind (the pattern of test_model_equals_zlib_on_damaged_streams): where the model accepts,
    zlib accepts, with the same bytes and members"""
    rnd = random.Random(17)
    good = cases.good_cases()
    rows = [good[n][0] for n in ("fname", "fextra_fname_fcomment", "chain_of_2", "chain_of_3", "chain_empty_middle", "fname_and_fcomment_of_200")]
    small = cases.fasta_text(1500, 23)
    rows += [cases.member(cases.raw_deflate(small, lv, st), small) for lv, st in ((6, zlib.Z_FIXED), (6, zlib.Z_HUFFMAN_ONLY), (0, zlib.Z_DEFAULT_STRATEGY))]
    accepted = refused = copies = 0
    for row in rows:
        for _ in range(40):
            at = rnd.randrange(min(len(row), 120)) if rnd.random() < 0.7 else rnd.randrange(len(row))
            bad = bytearray(row)
            bad[at] ^= 1 << rnd.randrange(8)
            copies += 1
            z = zlib_chain(bytes(bad))
            try:
                got = ref.inflate_row(bytes(bad), 1 << 20)
                assert z == got
                accepted += 1
            except ref.Refused:
                refused += 1
    assert copies >= 300 and accepted > 20 and refused > 100


def hint_of(buf, n, info):
    assert api.lib().mc_gzip_hint(buf.ctypes.data if n else None, n, info.ctypes.data) == 0
    return tuple(int(x) for x in info)


def test_gzip_hint_equals_the_models_header_walk():
    """every row; every prefix of every row below 4 KiB; of a longer row every prefix up to 600 bytes (the longest header here ends at
    412), 200 seeded lengths and the last 20 -- the walk reads the header and the last four bytes and nothing between"""
    info = np.zeros(4, dtype=np.uint64)
    rnd = random.Random(5)
    rows = [(n, r[0]) for n, r in cases.good_cases().items()] + [(n, r[0]) for n, r in cases.bad_cases().items()]
    for name, row in rows:
        # an exact heap block per row; lengths are taken from its front
        buf = np.frombuffer(row, dtype=np.uint8).copy()
        assert hint_of(buf, len(row), info) == ref.hint(row) == api.gzip_hint(row), name
        if len(row) < 4096:
            lengths = range(len(row))
        else:
            lengths = list(range(600)) + [rnd.randrange(600, len(row)) for _ in range(200)] + list(range(len(row) - 20, len(row)))
        for k in lengths:
            assert hint_of(buf, k, info) == ref.hint(row[:k]), f"{name}: prefix of {k}"
    good = cases.good_cases()
    assert api.gzip_hint(good["one_mib"][0]) == (api.GZIP_OK, 10, 1 << 20, 0)
    assert api.gzip_hint(good["fname"][0])[:2] == (api.GZIP_OK, 10 + len(b"genome.fna") + 1)
    assert api.gzip_hint(cases.bad_cases()["fhcrc"][0])[0::3] == (api.GZIP_FOREIGN, ref.R_HEADER)
    assert api.gzip_hint(b"") == (api.GZIP_FOREIGN, 0, 0, ref.R_INPUT)
    # a chain's trailing ISIZE is its last member's: too small, stated, and the call then ends in R_OVER for that row
    row, plain = good["chain_of_3"]
    assert api.gzip_hint(row)[2] < len(plain)
    with pytest.raises(ref.Refused) as e:
        ref.inflate_row(row, api.gzip_hint(row)[2])
    assert e.value.reason == ref.R_OVER
    L = api.lib()
    assert L.mc_gzip_hint(None, 0, None) == -1 and L.mc_gzip_hint(None, 5, info.ctypes.data) == -1


def test_names_exported_and_declared():
    with open(os.path.join(ROOT, "include", "metacache_amd.h")) as f:
        header = f.read()
    for name in ("mc_gzip_hint", "mc_inflate_streams", "mc_inflate_streams_stats"):
        assert name in api.EXPORTS and hasattr(api.lib(), name) and ("int " + name + "(") in header
    for k, v in dict(MC_GZIP_OK=api.GZIP_OK, MC_GZIP_FOREIGN=api.GZIP_FOREIGN, MC_INFLATE_R_HEADER=ref.R_HEADER, MC_INFLATE_R_TRAILING=ref.R_TRAILING).items():
        assert any(line.split()[:3] == ["#define", k, str(v)] for line in header.split("\n")), k
    assert (api.INFLATE_R_HEADER, api.INFLATE_R_TRAILING) == (ref.R_HEADER, ref.R_TRAILING)
    assert api.gzip_stream_dtype.itemsize == 32 and api.gzip_result_dtype.itemsize == 16
    with open(os.path.join(ROOT, "metacache_amd", "build.py")) as f:
        assert '"inflate_streams.hip"' in f.read()


def test_argument_checks_need_no_device():
    L = api.lib()
    h = C.c_void_p()
    assert L.mc_open_metadata(os.path.join(GOLDEN, "toy32").encode(), C.byref(h)) == api.MC_OK
    try:
        m, plain = cases.good_cases()["fname"]
        data = np.frombuffer(m + b"\0" * 16, dtype=np.uint8).copy()
        rows = np.array([(0, len(m), 0, len(plain))], dtype=api.gzip_stream_dtype)
        out = np.zeros(8192, dtype=np.uint8)
        results = np.zeros(4, dtype=api.gzip_result_dtype)
        status = np.zeros(4, dtype=np.uint64)
        buf = np.zeros(1 << 14, dtype=np.uint64)                    # (its addresses are only compared, never read: no device)
        base = buf.ctypes.data + (-buf.ctypes.data) % 16

        def call(ctx=h, bytes_ptr=data.ctypes.data, nbytes=len(m), rows_ptr=rows.ctypes.data, n=1, flags=api.INFLATE_HOST, out_ptr=out.ctypes.data, cap=len(plain),
                 results_ptr=results.ctypes.data, status_ptr=status.ctypes.data):
            return L.mc_inflate_streams(ctx, bytes_ptr, nbytes, rows_ptr, n, flags, out_ptr, cap, results_ptr, status_ptr, None)

        assert call(ctx=None) == -1
        assert call(bytes_ptr=None) == -1 and call(rows_ptr=None) == -1 and call(results_ptr=None) == -1 and call(status_ptr=None) == -1
        assert call(out_ptr=None) == -1
        assert call(flags=2) == -1 and call(flags=api.INFLATE_HOST | 4) == -1
        assert call(n=(1 << 30) + 1) == -1
        assert call(out_ptr=data.ctypes.data + 100, cap=50) == -1 and b"overlaps" in L.mc_last_error(h)

        # the rows of the host form are checked on the host: the limits, the range, disjoint slices
        def with_rows(r, nbytes=len(m)):
            a = np.array(r, dtype=api.gzip_stream_dtype)
            return call(rows_ptr=a.ctypes.data, n=len(a), nbytes=nbytes)
        assert with_rows([(0, len(m) + 1, 0, 10)]) == -1                      # beyond nbytes
        assert with_rows([(0, 17, 0, 10)]) == -1                              # in_len 17
        assert with_rows([(0, (1 << 28) + 1, 0, 10)], nbytes=1 << 29) == -1   # in_len beyond 2^28
        assert with_rows([(0, len(m), 0, (1 << 31) + 1)]) == -1               # out_cap beyond 2^31
        assert with_rows([(0, 100, 0, 10), (100, 100, 9, 10)]) == -1          # slices overlap
        assert with_rows([(0, 100, 20, 10), (100, 100, 0, 21)]) == -1         # ... in any order
        assert with_rows([(0, 100, 1 << 63, 1 << 31), (0, 100, (1 << 64) - 5, 10)]) == -1   # a slice that wraps
        assert b"row" in L.mc_last_error(h)
        # the device form: alignment, before any device call
        dev = dict(flags=0, bytes_ptr=base, rows_ptr=base + 4096, out_ptr=base + 8192, results_ptr=base + 12288, status_ptr=base + 16384)
        assert call(**{**dev, "bytes_ptr": base + 8}) == -1 and call(**{**dev, "out_ptr": base + 8200}) == -1
        assert call(**{**dev, "rows_ptr": base + 4100}) == -1 and call(**{**dev, "results_ptr": base + 12292}) == -1 and call(**{**dev, "status_ptr": base + 16388}) == -1
        assert b"aligned" in L.mc_last_error(h)
        # arguments in order: the context has no device
        assert call(**dev) == -6 and call() == -6 and call(n=0) == -6
        assert with_rows([(0, 100, 0, 10), (100, 100, 10, 10), (0, 100, 30, 0), (0, 100, 5, 0)]) == -6      # disjoint; empty slices overlap nothing
        assert b"no device" in L.mc_last_error(h)
        assert not status.any() and not out.any() and not results.view(np.uint8).any()
        st = np.ones(4, dtype=np.uint64)
        assert L.mc_inflate_streams_stats(h, st.ctypes.data) == 0 and not st.any()
        assert L.mc_inflate_streams_stats(h, None) == -1 and L.mc_inflate_streams_stats(None, st.ctypes.data) == -1
    finally:
        L.mc_destroy(h)
