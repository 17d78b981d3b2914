"""Seeded BGZF members for the inflate tests (standard library only): good members of every block type and shape the decoder has a path
for, and members that must be refused.  good_cases() / bad_cases() build them once; a case is (member bytes, plain bytes)."""
import functools
import random
import struct
import zlib

PAYLOAD = 65280      # bgzip's payload size


def member(deflate, plain=None, *, crc=None, isize=None, extra=b""):
    """a BGZF member around a raw deflate stream; crc / isize default to those of `plain`; extra: subfields in front of BC"""
    xtra = extra + b"BC\x02\x00" + struct.pack("<H", 12 + len(extra) + 6 + len(deflate) + 8 - 1)
    crc = zlib.crc32(plain) if crc is None else crc
    isize = len(plain) if isize is None else isize
    return b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", len(xtra)) + xtra + deflate + struct.pack("<II", crc & 0xFFFFFFFF, isize)


def bgzf_block(payload, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if flush_at is None:
        raw = c.compress(payload) + c.flush()
    else:
        raw = c.compress(payload[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(payload[flush_at:]) + c.flush()
    return member(raw, payload)


EOF_BLOCK = bgzf_block(b"")
assert len(EOF_BLOCK) == 28


def bgzf_file(data, level=6, eof=True, payload=PAYLOAD):
    return b"".join(bgzf_block(data[i:i + payload], level) for i in range(0, len(data), payload)) + (EOF_BLOCK if eof else b"")


def fastq_text(nbytes, seed):
    rnd = random.Random(seed)
    parts, n, i = [], 0, 0
    while n < nbytes:
        L = rnd.randint(100, 151)
        rec = "@read%d/%d\n%s\n+\n%s\n" % (i, seed, "".join(rnd.choice("ACGT") for _ in range(L)), "".join(rnd.choice("FFFFF:,#") for _ in range(L)))
        parts.append(rec.encode())
        n += len(rec)
        i += 1
    return b"".join(parts)[:nbytes]


def fibonacci_payload(seed=5, nbytes=PAYLOAD):
    """byte frequencies that are Fibonacci numbers (as many as fit, the rest of the bytes to one more symbol), shuffled: the deepest
    Huffman tree for its size, so Z_HUFFMAN_ONLY runs into the 15-bit limit"""
    fib = [1, 1]
    while sum(fib) + fib[-1] + fib[-2] <= nbytes:
        fib.append(fib[-1] + fib[-2])
    fib.append(nbytes - sum(fib))
    pool = [65 + s for s, n in enumerate(fib) for _ in range(n)]
    random.Random(seed).shuffle(pool)
    return bytes(pool)


# ---- a fixed-Huffman emitter: chosen (length, distance) pairs --------------------------------------------
class Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, x, n):          # n bits of x, lowest first
        self.v |= (x & ((1 << n) - 1)) << self.n
        self.n += n

    def code(self, c, n):         # a Huffman code: highest bit first
        for i in range(n - 1, -1, -1):
            self.put((c >> i) & 1, 1)

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


class Fixed(Bits):
    def __init__(self, last=1):
        super().__init__()
        self.put(last, 1)
        self.put(1, 2)

    def sym(self, s):
        if s < 144: self.code(0x30 + s, 8)
        elif s < 256: self.code(0x190 + s - 144, 9)
        elif s < 280: self.code(s - 256, 7)
        else: self.code(0xC0 + s - 280, 8)

    def dcode(self, d):
        self.code(d, 5)

    def match(self, length, dist):
        k = max(i for i in range(29) if LBASE[i] <= length) if length < 258 else 28
        self.sym(257 + k)
        self.put(length - LBASE[k], LEXT[k])
        k = max(i for i in range(30) if DBASE[i] <= dist)
        self.dcode(k)
        self.put(dist - DBASE[k], DEXT[k])

    def fill(self, upto, pos):    # matches at distance 1 from pos up to `upto`, none shorter than 3
        while pos < upto:
            n = min(258, upto - pos)
            if 0 < upto - pos - n < 3:
                n -= 3
            self.match(n, 1)
            pos += n

    def end(self):
        self.sym(256)
        return self.bytes()


def far_match_stream():
    """one literal, fills at distance 1 up to 32 768, a match of 258 at distance 32 768, 3 at 32 768, 258 at distance 2, 5 at distance 3"""
    f = Fixed()
    f.sym(ord("x"))
    f.fill(32768, 1)
    out = bytearray(b"x" * 32768)
    for n, d in ((258, 32768), (3, 32768), (258, 2), (5, 3)):
        f.match(n, d)
        for i in range(n):
            out.append(out[len(out) - d])
    return f.end(), bytes(out)


def dynamic_header(cl_lens, hlit=0, hdist=0, last=1):
    """a dynamic block's header up to the code-length code, cl_lens = {symbol: length}; the writer is left behind it"""
    order = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
    ncl = max(4, 1 + max(order.index(s) for s in cl_lens))
    b = Bits()
    b.put(last, 1); b.put(2, 2); b.put(hlit, 5); b.put(hdist, 5); b.put(ncl - 4, 4)
    for s in order[:ncl]:
        b.put(cl_lens.get(s, 0), 3)
    return b


@functools.lru_cache(maxsize=None)
def good_cases():
    """name -> (member, plain)"""
    text = fastq_text(2 * PAYLOAD, 11)
    a, b2 = text[:PAYLOAD], text[PAYLOAD:]
    rnd = random.Random(3)
    noise = bytes(rnd.getrandbits(8) for _ in range(PAYLOAD))
    text_max = fastq_text(65536, 13)
    fib = fibonacci_payload()
    far, far_plain = far_match_stream()
    zeros = bytes(65536)
    c = {
        "eof": (EOF_BLOCK, b""),
        "stored_level0": (bgzf_block(a, 0), a),
        "fixed": (bgzf_block(a, 6, zlib.Z_FIXED), a),
        "dynamic_l1": (bgzf_block(a, 1), a),
        "dynamic_l6": (bgzf_block(b2, 6), b2),
        "dynamic_l9": (bgzf_block(a, 9), a),
        "dynamic_rle": (bgzf_block(b2, 6, zlib.Z_RLE), b2),
        "dynamic_huffman_only": (bgzf_block(a, 6, zlib.Z_HUFFMAN_ONLY), a),
        "two_blocks_flush": (bgzf_block(a, 6, flush_at=30011), a),
        "fibonacci_15bit": (bgzf_block(fib, 6, zlib.Z_HUFFMAN_ONLY), fib),
        "far_match": (member(far, far_plain), far_plain),
        "largest_expansion": (bgzf_block(zeros, 9), zeros),
        "noise_stored": (bgzf_block(noise, 6), noise),
        "largest_isize": (bgzf_block(text_max, 6), text_max),
        "short_text": (bgzf_block(a[:1234], 6), a[:1234]),
        "one_byte": (bgzf_block(b"A", 6), b"A"),
        "bc_behind_another_subfield": (member(zlib.compress(a[:777])[2:-4], a[:777], extra=b"XY\x03\x00abc"), a[:777]),
    }
    return c


@functools.lru_cache(maxsize=None)
def bad_cases():
    """name -> member that must be refused (the first six by zlib too, the next three as well; the last four by the trailer rules)"""
    good, plain = good_cases()["dynamic_l6"]
    import inflate_ref
    pay = inflate_ref.payload_of(good)
    small = fastq_text(3000, 7)
    spay = inflate_ref.payload_of(bgzf_block(small, 6))
    x = {}
    x["block_type_3"] = member(b"\x07\x00", b"")
    x["stored_len_nlen"] = member(b"\x01\x05\x00\xfb\xffhello", b"hello")
    f = Fixed(); f.sym(65); f.match(3, 5)
    x["distance_beyond_output"] = member(f.end(), b"AAAA")
    f = Fixed(); f.sym(65); f.sym(286)
    x["symbol_286"] = member(f.end(), b"A")
    f = Fixed(); f.sym(65); f.sym(257); f.dcode(30)
    x["distance_code_30"] = member(f.end(), b"AAAA")
    x["cut_in_half"] = member(pay[:len(pay) // 2], plain)
    h = dynamic_header({16: 1, 17: 1, 18: 1, 0: 1})
    x["oversubscribed_code_lengths"] = member(h.bytes() + b"\x00\x00", b"")
    h = dynamic_header({16: 1, 0: 1}); h.code(1, 1); h.put(0, 2)
    x["repeat_16_first"] = member(h.bytes() + b"\x00\x00", b"")
    h = dynamic_header({18: 1, 0: 1}); h.code(1, 1); h.put(127, 7); h.code(1, 1); h.put(127, 7)
    x["repeat_past_the_end"] = member(h.bytes() + b"\x00\x00", b"")
    x["wrong_crc"] = member(spay, small, crc=zlib.crc32(small) ^ 0x8000)
    x["isize_one_too_large"] = member(spay, small, isize=len(small) + 1)
    x["isize_one_too_small"] = member(spay, small, isize=len(small) - 1)
    x["spare_byte"] = member(spay + b"\x00", small)
    return x


ZLIB_REFUSES = ("block_type_3", "stored_len_nlen", "distance_beyond_output", "symbol_286", "distance_code_30", "cut_in_half",
                "oversubscribed_code_lengths", "repeat_16_first", "repeat_past_the_end")
