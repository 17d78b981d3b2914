"""The stream rule of include/metacache_amd.h (whole gzip files) restated in plain Python: the header of a member
(header_at), the chain of members of a row (inflate_row), what mc_gzip_hint owes (hint) and what mc_inflate_streams owes for a set of
rows (expected).  One deflate stream is inflate_ref.inflate_stream, the block rule's; only its bit reader is exchanged for the time of a
call, for one that does not shift the whole payload per symbol (a megabyte member would take minutes).  The oracle of all of this is
zlib (tests/test_gzip_witness_cpu.py).  The order of the checks is the kernel's."""
import contextlib
import struct
import zlib

import inflate_ref
from inflate_ref import (INFLATE_CORRUPT, INFLATE_OK, INFLATE_OVERFLOW, R_BTYPE, R_CRC, R_DISTANCE, R_INPUT, R_LENGTHS, R_OVER, R_SHORT,  # noqa: F401
                         R_STORED, R_SYMBOL)

R_HEADER, R_TRAILING = 11, 12
REASONS = dict(inflate_ref.REASONS)
REASONS.update({R_HEADER: "header", R_TRAILING: "trailing bytes"})
GZIP_OK, GZIP_FOREIGN = 0, 1
MIN_ROW, MAX_ROW_IN, MAX_ROW_OUT = 18, 1 << 28, 1 << 31


class Refused(Exception):
    def __init__(self, reason, members=0):
        super().__init__(REASONS[reason])
        self.reason, self.members = reason, members


class _WindowBits(inflate_ref._Bits):
    """inflate_ref._Bits with the same answers, reading eight bytes at the place instead of shifting the whole payload"""

    def __init__(self, data):
        self.data, self.pos, self.left = bytes(data), 0, 8 * len(data)

    def peek(self, n):
        at = self.pos >> 3
        v = int.from_bytes(self.data[at:at + 8], "little") >> (self.pos & 7)
        return v & ((1 << min(n, self.left)) - 1)


@contextlib.contextmanager
def _window_bits():
    keep = inflate_ref._Bits
    inflate_ref._Bits = _WindowBits
    try:
        yield
    finally:
        inflate_ref._Bits = keep


def inflate_stream(payload, limit):
    """inflate_ref.inflate_stream: -> (bytes, bytes left behind the stream, features); raises inflate_ref.Refused"""
    with _window_bits():
        return inflate_ref.inflate_stream(payload, limit)


def header_at(row, p, first):
    """the header of the member at row[p], p < len(row): the offset of its deflate stream.  Raises Refused"""
    n = len(row)
    if n - p < 2 or row[p:p + 2] != b"\x1f\x8b":
        raise Refused(R_HEADER if first else R_TRAILING)
    if n - p < 10 or row[p + 2] != 8:
        raise Refused(R_HEADER)
    flg = row[p + 3]
    if flg & 0xE2:
        raise Refused(R_HEADER)
    at = p + 10
    if flg & 4:
        if n - at < 2:
            raise Refused(R_HEADER)
        xlen = struct.unpack_from("<H", row, at)[0]
        if n - at - 2 < xlen:
            raise Refused(R_HEADER)
        at += 2 + xlen
    for bit in (8, 16):
        if flg & bit:
            z = row.find(b"\x00", at)
            if z < 0:
                raise Refused(R_HEADER)
            at = z + 1
    return at


def inflate_row(row, out_cap):
    """the bytes of one row by the stream rule -> (bytes, members).  Raises Refused(reason, members finished)"""
    row = bytes(row)
    n = len(row)
    if n < MIN_ROW or n > MAX_ROW_IN or out_cap > MAX_ROW_OUT:
        raise Refused(R_INPUT)
    out, p, members = [], 0, 0
    total = 0
    try:
        while True:
            pay = header_at(row, p, members == 0)
            if n - pay < 8:
                raise Refused(R_INPUT)
            try:
                plain, left, _ = inflate_stream(row[pay:n - 8], out_cap - total)
            except inflate_ref.Refused as e:
                raise Refused(e.reason)
            trailer = n - 8 - left
            crc, isize = struct.unpack_from("<II", row, trailer)
            if len(plain) != isize:
                raise Refused(R_SHORT if len(plain) < isize else R_OVER)
            if zlib.crc32(plain) != crc:
                raise Refused(R_CRC)
            out.append(plain)
            total += len(plain)
            members += 1
            p = trailer + 8
            if p == n:
                return b"".join(out), members
    except Refused as e:
        raise Refused(e.reason, members)


def hint(data):
    """what mc_gzip_hint owes: (verdict, the offset of the first deflate stream, the trailing ISIZE, the offence)"""
    data = bytes(data)
    isize = struct.unpack_from("<I", data, len(data) - 4)[0] if len(data) >= 4 else 0
    if len(data) < MIN_ROW:
        return GZIP_FOREIGN, 0, isize, R_INPUT
    try:
        pay = header_at(data, 0, True)
        if len(data) - pay < 8:
            raise Refused(R_INPUT)
    except Refused as e:
        return GZIP_FOREIGN, 0, isize, e.reason
    return GZIP_OK, pay, isize, 0


def expected(data, rows, out_capacity, known=None):
    """what mc_inflate_streams owes for rows [(in_off, in_len, out_off, out_cap)]: (status [verdict, lowest refused row, reason, accepted
    rows], results [(produced, members, reason)], {row: bytes}).  known: {row bytes: inflate_row's answer or its Refused}, filled and used"""
    known = {} if known is None else known
    results, good, bad = [], {}, None
    for i, (in_off, in_len, out_off, out_cap) in enumerate(rows):
        try:
            if out_off + out_cap > out_capacity:
                raise Refused(R_OVER)
            if in_off + in_len > len(data):
                raise Refused(R_INPUT)
            key = (bytes(data[in_off:in_off + in_len]), out_cap)
            if key not in known:
                try:
                    known[key] = inflate_row(key[0], out_cap)
                except Refused as e:
                    known[key] = e
            if isinstance(known[key], Refused):
                raise Refused(known[key].reason, known[key].members)
            good[i] = known[key][0]
            results.append((len(good[i]), known[key][1], 0))
        except Refused as e:
            results.append((0, e.members, e.reason))
            if bad is None:
                bad = (INFLATE_OVERFLOW if e.reason == R_OVER else INFLATE_CORRUPT, i, e.reason)
    status = [INFLATE_OK, 0, 0, len(good)] if bad is None else [bad[0], bad[1], bad[2], len(good)]
    return status, results, good
