"""The BGZF rule of include/metacache_amd.h restated in plain Python: the walk over the members (walk), a plain inflate of one deflate
stream (inflate_stream) that also reports what the stream contains, the member with its trailer rules (inflate_member) and the status
mc_inflate_blocks owes for a set of rows (expected_status).  The oracle of all of this is zlib (tests/test_inflate_witness_cpu.py);
this file exists so that the refusals have a reason and the cases can say what they cover.  The order of the checks is the kernel's."""
import struct
import zlib

BGZF_OK, BGZF_FOREIGN = 0, 1
INFLATE_OK, INFLATE_CORRUPT, INFLATE_OVERFLOW = 0, 1, 2
R_BTYPE, R_STORED, R_LENGTHS, R_SYMBOL, R_DISTANCE, R_INPUT, R_OVER, R_SHORT, R_LEFT, R_CRC = range(1, 11)
REASONS = {1: "block type", 2: "stored lengths", 3: "code lengths", 4: "symbol", 5: "distance", 6: "overrun of the input", 7: "overrun of ISIZE",
           8: "short of ISIZE", 9: "bytes left before the trailer", 10: "crc"}
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


class Refused(Exception):
    def __init__(self, reason):
        super().__init__(REASONS[reason])
        self.reason = reason


# ---- the members ---------------------------------------------------------------------------------
def member_at(data, p):
    """the member at offset p: (size, isize), or None"""
    n = len(data)
    if n - p < 12 or data[p:p + 4] != b"\x1f\x8b\x08\x04":
        return None
    xlen = struct.unpack_from("<H", data, p + 10)[0]
    if n - p - 12 < xlen:
        return None
    at, bsize = 0, None
    while at < xlen:
        if xlen - at < 4:
            return None
        f = p + 12 + at
        slen = struct.unpack_from("<H", data, f + 2)[0]
        if xlen - at - 4 < slen:
            return None
        if data[f:f + 2] == b"BC":
            if slen != 2 or bsize is not None:
                return None
            bsize = struct.unpack_from("<H", data, f + 4)[0]
        at += 4 + slen
    if bsize is None:
        return None
    size = bsize + 1
    if size < 12 + xlen + 8 or n - p < size:
        return None
    isize = struct.unpack_from("<I", data, p + size - 4)[0]
    return (size, isize) if isize <= 65536 else None


def walk(data):
    """-> (rows [(in_off, out_off, in_len, out_len)], out_bytes, verdict, offence): what mc_bgzf_index owes"""
    rows, p, out = [], 0, 0
    if len(data) == 0:
        return rows, 0, BGZF_FOREIGN, 0
    while p < len(data):
        m = member_at(data, p)
        if m is None:
            return rows, out, BGZF_FOREIGN, p
        rows.append((p, out, m[0], m[1]))
        out += m[1]
        p += m[0]
    return rows, out, BGZF_OK, 0


def payload_of(member):
    xlen = struct.unpack_from("<H", member, 10)[0]
    return member[12 + xlen:len(member) - 8]


# ---- one deflate stream ------------------------------------------------------------------------------
class _Bits:
    def __init__(self, data):
        self.v = int.from_bytes(data, "little")
        self.pos = 0
        self.left = 8 * len(data)

    def peek(self, n):      # the next n bits, those beyond the payload as zeros
        return (self.v >> self.pos) & ((1 << min(n, self.left)) - 1)

    def need(self, n):
        if n > self.left:
            raise Refused(R_INPUT)

    def drop(self, n):
        self.pos += n
        self.left -= n

    def take(self, n):
        self.need(n)
        x = self.peek(n)
        self.drop(n)
        return x


class _Code:
    """a canonical code set: count per length, symbols by (length, symbol)"""
    def __init__(self, lens):
        self.cnt = [0] * 16
        for l in lens:
            self.cnt[l] += 1
        self.cnt[0] = 0
        self.sym = [s for l in range(1, 16) for s, x in enumerate(lens) if x == l]
        left, self.over = 1, False
        for l in range(1, 16):
            left = 2 * left - self.cnt[l]
            if left < 0:
                self.over, left = True, 0
        self.incomplete = left > 0
        self.max = max([l for l in range(1, 16) if self.cnt[l]] or [0])

    def decode(self, v, maxbits=15):
        """(symbol, length) of the code the low bits of v begin with, or None"""
        code = first = index = 0
        for l in range(1, maxbits + 1):
            code |= v & 1
            v >>= 1
            c = self.cnt[l]
            if code < first + c:
                return self.sym[index + code - first], l
            index += c
            first = (first + c) << 1
            code <<= 1
        return None


def inflate_stream(payload, limit=1 << 32):
    """-> (bytes, bytes left behind the stream, features).  Raises Refused(reason).  features: types (the block types in order), longest_code,
    max_dist, min_dist, longest_match, overlaps (copies with distance < length)"""
    b = _Bits(payload)
    out = bytearray()
    f = dict(types=[], longest_code=0, max_dist=0, min_dist=None, longest_match=0, overlaps=0)
    while True:
        head = b.take(3)
        last, typ = head & 1, head >> 1
        if typ == 3:
            raise Refused(R_BTYPE)
        f["types"].append(typ)
        if typ == 0:
            b.drop(b.left & 7)
            v = b.take(32)
            n = v & 0xFFFF
            if (n ^ 0xFFFF) != v >> 16:
                raise Refused(R_STORED)
            b.need(8 * n)
            if n > limit - len(out):
                raise Refused(R_OVER)
            at = len(payload) - b.left // 8
            out += payload[at:at + n]
            b.drop(8 * n)
        else:
            if typ == 1:
                lens = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8 + [5] * 32
                nlit = 288
            else:
                h = b.take(14)
                nlit, ndist, ncl = (h & 31) + 257, ((h >> 5) & 31) + 1, (h >> 10) + 4
                if nlit > 286 or ndist > 30:
                    raise Refused(R_LENGTHS)
                cl = [0] * 19
                for i in range(ncl):
                    cl[CL_ORDER[i]] = b.take(3)
                clc = _Code(cl)
                if clc.over or clc.incomplete:
                    raise Refused(R_LENGTHS)
                lens, prev = [], 0
                while len(lens) < nlit + ndist:
                    d = clc.decode(b.peek(7), 7)
                    if d is None:
                        raise Refused(R_LENGTHS)
                    b.need(d[1])
                    b.drop(d[1])
                    s = d[0]
                    if s < 16:
                        lens.append(s)
                        prev = s
                        continue
                    if s == 16 and not lens:
                        raise Refused(R_LENGTHS)
                    rep = (3 if s < 18 else 11) + b.take(2 if s == 16 else 3 if s == 17 else 7)
                    if rep > nlit + ndist - len(lens):
                        raise Refused(R_LENGTHS)
                    val = prev if s == 16 else 0
                    lens += [val] * rep
                    prev = val
                if lens[256] == 0:
                    raise Refused(R_LENGTHS)
            lit, dst = _Code(lens[:nlit]), _Code(lens[nlit:])
            if lit.over or (lit.incomplete and lit.max != 1):
                raise Refused(R_LENGTHS)
            if dst.over or (dst.incomplete and dst.max > 1):
                raise Refused(R_LENGTHS)
            f["longest_code"] = max(f["longest_code"], lit.max, dst.max)
            while True:
                d = lit.decode(b.peek(15))
                if d is None:
                    raise Refused(R_SYMBOL if b.left else R_INPUT)
                b.need(d[1])
                b.drop(d[1])
                s = d[0]
                if s < 256:
                    if len(out) >= limit:
                        raise Refused(R_OVER)
                    out.append(s)
                    continue
                if s == 256:
                    break
                if s >= 286:
                    raise Refused(R_SYMBOL)
                if s < 265:
                    n = s - 254
                elif s == 285:
                    n = 258
                else:
                    xb = (s - 261) >> 2
                    n = ((4 + ((s - 265) & 3)) << xb) + 3 + b.take(xb)
                d = dst.decode(b.peek(15))
                if d is None:
                    raise Refused(R_DISTANCE if b.left else R_INPUT)
                b.need(d[1])
                b.drop(d[1])
                ds = d[0]
                if ds >= 30:
                    raise Refused(R_DISTANCE)
                if ds < 4:
                    dist = ds + 1
                else:
                    xb = (ds >> 1) - 1
                    dist = ((2 + (ds & 1)) << xb) + 1 + b.take(xb)
                if dist > len(out):
                    raise Refused(R_DISTANCE)
                if n > limit - len(out):
                    raise Refused(R_OVER)
                pos = len(out)
                for i in range(n):
                    out.append(out[pos - dist + i % dist])
                f["max_dist"] = max(f["max_dist"], dist)
                f["min_dist"] = dist if f["min_dist"] is None else min(f["min_dist"], dist)
                f["longest_match"] = max(f["longest_match"], n)
                f["overlaps"] += dist < n
        if last:
            break
    b.drop(b.left & 7)
    return bytes(out), b.left // 8, f


def inflate_member(member, out_len=None):
    """the bytes of one member by the block rule; out_len: the row's (default: the trailer's ISIZE).  Raises Refused(reason)"""
    crc, isize = struct.unpack_from("<II", member, len(member) - 8)
    out, left, _ = inflate_stream(payload_of(member), isize if out_len is None else out_len)
    if left:
        raise Refused(R_LEFT)
    if len(out) != isize:
        raise Refused(R_SHORT if len(out) < isize else R_OVER)
    if zlib.crc32(out) != crc:
        raise Refused(R_CRC)
    return out


def expected_status(data, rows, out_capacity):
    """what mc_inflate_blocks owes for these rows: ([verdict, lowest bad row, reason, bytes covered], {row: bytes})"""
    covered, good = 0, {}
    bad = None
    for i, (in_off, out_off, in_len, out_len) in enumerate(rows):
        if out_off + out_len > out_capacity:
            if bad is None:
                bad = (INFLATE_OVERFLOW, i, 0)
            continue
        covered = max(covered, out_off + out_len)
        try:
            if in_off + in_len > len(data) or in_len < 20 or in_len < 20 + struct.unpack_from("<H", data, in_off + 10)[0]:
                raise Refused(R_INPUT)
            good[i] = inflate_member(data[in_off:in_off + in_len], out_len)
        except Refused as e:
            if bad is None:
                bad = (INFLATE_CORRUPT, i, e.reason)
    return ([INFLATE_OK, 0, 0, covered] if bad is None else [bad[0], bad[1], bad[2], covered]), good
