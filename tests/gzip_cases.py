"""Seeded gzip rows for the stream tests (standard library only): good rows for every path the stream decoder has beyond the block
decoder's -- positions beyond 2^16, many blocks, general headers, chains of members -- and rows that must be refused, each named for its
reason.  good_cases(): name -> (row bytes, plain bytes).  bad_cases(): name -> (row bytes, out_cap, reason).  Built once.
The emitters are inflate_cases' (Fixed: chosen length / distance pairs in a fixed-Huffman block)."""
import functools
import random
import struct
import zlib

import gzip_ref as ref
from inflate_cases import Fixed

FTEXT, FHCRC, FEXTRA, FNAME, FCOMMENT = 1, 2, 4, 8, 16


def member(deflate, plain, *, flg=0, extra=None, name=None, comment=None, crc=None, isize=None, cm=8, magic=b"\x1f\x8b", hcrc=False):
    """a gzip member around a raw deflate stream; the optional fields set their FLG bits; crc / isize default to those of `plain`"""
    flg |= (FEXTRA if extra is not None else 0) | (FNAME if name is not None else 0) | (FCOMMENT if comment is not None else 0) | (FHCRC if hcrc else 0)
    h = magic + bytes([cm, flg]) + b"\x00\x00\x00\x00\x00\x03"
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\x00"
    if comment is not None:
        h += comment + b"\x00"
    if hcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    crc = zlib.crc32(plain) if crc is None else crc
    isize = len(plain) if isize is None else isize
    return h + deflate + struct.pack("<II", crc & 0xFFFFFFFF, isize & 0xFFFFFFFF)


def raw_deflate(plain, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if flush_every is None:
        return c.compress(plain) + c.flush()
    parts = []
    for at in range(0, len(plain), flush_every):
        parts.append(c.compress(plain[at:at + flush_every]) + c.flush(zlib.Z_FULL_FLUSH))      # (ends in an empty stored block)
    return b"".join(parts) + c.flush()


def stored_blocks(plain, size=65535):
    """a stream of stored blocks of `size` bytes, the largest a stored block holds, and one of what is left (not every zlib writes these)"""
    parts = []
    for at in range(0, len(plain), size):
        piece = plain[at:at + size]
        parts.append(bytes([1 if at + size >= len(plain) else 0]) + struct.pack("<HH", len(piece), len(piece) ^ 0xFFFF) + piece)
    return b"".join(parts)


def gz(plain, level=6, **kw):
    return member(raw_deflate(plain, level), plain, **kw)


def fasta_text(nbytes, seed, repeats=False):
    """a genome file's text: a header line and lines of 80 bases; repeats: most of it is earlier text again with a base changed here and
    there, so that the stream is long matches at far distances"""
    rnd = random.Random(seed)
    parts, n, i = [], 0, 0
    base = None
    while n < nbytes:
        hdr = ">NC_%06d.%d synthetic sequence %d\n" % (seed, i, i)
        if repeats and base is not None:
            s = bytearray(base)
            for _ in range(len(s) // 211):
                s[rnd.randrange(len(s))] = rnd.choice(b"ACGT")
            seq = s.decode()
        else:
            seq = "".join(rnd.choice("ACGT") for _ in range(rnd.randint(18000, 24000)))
            base = seq.encode()
        body = "\n".join(seq[k:k + 80] for k in range(0, len(seq), 80)) + "\n"
        parts.append((hdr + body).encode())
        n += len(parts[-1])
        i += 1
    return b"".join(parts)[:nbytes]


def straddle_stream(length, dist, start):
    """a fixed-Huffman stream whose match (length, dist) begins at output position `start`: 300 mixed literals, a fill at distance 1 up to
    32 768, matches at distance 32 768 up to `start`, the match, three literals -> (deflate, plain)"""
    rnd = random.Random(start * 1000 + length)
    f = Fixed()
    out = bytearray()
    for _ in range(300):
        s = rnd.randrange(256)
        f.sym(s)
        out.append(s)
    f.fill(32768, len(out))
    out += bytes([out[-1]]) * (32768 - len(out))

    def match(n, d):
        f.match(n, d)
        for _ in range(n):
            out.append(out[len(out) - d])

    while len(out) < start:
        n = min(258, start - len(out))
        if 0 < start - len(out) - n < 3:
            n -= 3
        match(n, 32768)
    match(length, dist)
    for s in b"end":
        f.sym(s)
        out.append(s)
    return f.end(), bytes(out)


@functools.lru_cache(maxsize=None)
def good_cases():
    """name -> (row, plain)"""
    text = fasta_text(200000, 3)
    small = fasta_text(3000, 5)
    tiny = fasta_text(700, 6)
    rnd = random.Random(9)
    noise = bytes(rnd.getrandbits(8) for _ in range(200000))
    big = fasta_text(256 << 10, 7) + fasta_text(768 << 10, 8, repeats=True)
    assert len(big) == 1 << 20
    c = {}
    c["one_member_200000"] = (gz(text), text)
    for what, (n, d, at) in {"match_258_at_32768_across_65536": (258, 32768, 65536 - 100), "match_3_at_32768_across_65536": (3, 32768, 65535),
                             "fill_at_1_across_65536": (258, 1, 65536 - 129)}.items():
        s, plain = straddle_stream(n, d, at)
        assert at < 65536 < at + n
        c[what] = (member(s, plain), plain)
    c["full_flush_pieces"] = (member(raw_deflate(text[:150000], 6, flush_every=7001), text[:150000]), text[:150000])
    c["stored_65535_in_a_row"] = (member(stored_blocks(noise), noise), noise)
    c["one_mib"] = (gz(big), big)
    c["fname"] = (gz(small, name=b"genome.fna"), small)
    c["fcomment"] = (gz(small, comment=b"a comment"), small)
    c["fextra"] = (gz(small, extra=b"XY\x03\x00abc"), small)
    c["fextra_fname_fcomment"] = (gz(small, extra=b"AB\x00\x00", name=b"more.fa", comment=b"from a test"), small)
    c["ftext"] = (gz(small, flg=FTEXT), small)
    c["fname_zero_at_byte_63_of_a_round"] = (gz(tiny, name=b"n" * 63), tiny)        # the header walk looks at 64 bytes per round
    c["fname_zero_in_the_next_round"] = (gz(tiny, name=b"n" * 64), tiny)
    c["fname_and_fcomment_of_200"] = (gz(tiny, name=b"p" * 200, comment=b"q" * 200), tiny)
    c["empty_file"] = (gz(b""), b"")
    a, b2, c3 = small[:1000], small[1000:1800], small[1800:]
    c["chain_of_2"] = (gz(a) + gz(b2, name=b"second"), a + b2)
    c["chain_of_3"] = (gz(a) + gz(b2, 1) + gz(c3, 9), small)
    c["chain_empty_first"] = (gz(b"") + gz(a) + gz(b2), a + b2)
    c["chain_empty_middle"] = (gz(a) + gz(b"") + gz(b2), a + b2)
    c["chain_empty_last"] = (gz(a) + gz(b2) + gz(b""), a + b2)
    c["chain_second_member_repeats_the_first"] = (gz(a) + gz(a), a + a)
    return c


@functools.lru_cache(maxsize=None)
def bad_cases():
    """name -> (row, out_cap, reason)"""
    small = fasta_text(3000, 5)
    a, b2 = small[:1000], small[1000:1800]
    d = raw_deflate(a)
    x = {}
    x["fhcrc"] = (gz(a, hcrc=True), len(a), ref.R_HEADER)
    x["reserved_flag"] = (gz(a, flg=0x20), len(a), ref.R_HEADER)
    x["cm_not_8"] = (gz(a, cm=7), len(a), ref.R_HEADER)
    x["bad_magic"] = (gz(a, magic=b"\x1f\x8c"), len(a), ref.R_HEADER)
    whole = gz(a, name=b"n" * 100)
    x["fname_without_zero"] = (whole[:60], len(a), ref.R_HEADER)
    x["fextra_past_the_row"] = (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\x03\xff\xff" + bytes(20), 0, ref.R_HEADER)
    x["truncated_stream"] = (member(d[:len(d) // 2], a), len(a), ref.R_INPUT)
    x["truncated_trailer"] = (gz(a)[:-3], len(a), ref.R_INPUT)
    x["header_then_no_room_for_a_trailer"] = (gz(b"", name=b"n" * 20)[:35], 0, ref.R_INPUT)
    x["trailing_zeros"] = (gz(a) + bytes(16), len(a), ref.R_TRAILING)
    x["trailing_garbage"] = (gz(a) + b"garbage behind the trailer", len(a), ref.R_TRAILING)
    x["trailing_single_byte"] = (gz(a) + b"\x1f", len(a), ref.R_TRAILING)
    x["wrong_crc_in_the_first_of_two"] = (member(d, a, crc=zlib.crc32(a) ^ 0x8000) + gz(b2), len(a) + len(b2), ref.R_CRC)
    x["wrong_isize_too_large"] = (member(d, a, isize=len(a) + 1), len(a) + 1, ref.R_SHORT)
    x["wrong_isize_too_small"] = (member(d, a, isize=len(a) - 1), len(a), ref.R_OVER)
    f = Fixed(); f.sym(65); f.match(3, 5)
    x["second_member_reaches_into_the_first"] = (gz(a) + member(f.end(), b"A" + a[-4:-1]), len(a) + 4, ref.R_DISTANCE)
    x["out_cap_one_short"] = (gz(a), len(a) - 1, ref.R_OVER)
    x["out_cap_one_short_in_the_second_member"] = (gz(a) + gz(b2), len(a) + len(b2) - 1, ref.R_OVER)
    x["in_len_17"] = (gz(b"")[:17], 0, ref.R_INPUT)
    x["block_type_3"] = (member(b"\x07\x00", b""), 0, ref.R_BTYPE)
    return x


# the host form refuses these rows as arguments (MC_ERR_INVALID) before any device call
HOST_ARGUMENT_ERRORS = ("in_len_17",)
