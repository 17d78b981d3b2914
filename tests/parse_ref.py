"""The record rule of mc_parse_records (include/metacache_amd.h) in plain Python: the model the device parse is held to.

A range is bytes B[0, n); B[0] is '>' (FASTA) or '@' (FASTQ).  A line start is position 0 or the byte after a '\\n'; trimmed = without
the trailing run of '\\r' / '\\n'.  parse(data) -> Parsed(verdict, offence, records) with records = [(hdr_off, hdr_len, seq bytes)];
the verdict is OK or IRREGULAR, the offence the offset of the first line start that broke the rule (len(data) for an incomplete last
FASTQ group).  pack(...) lays the records out as mc_parse_records does: qinfo, the packed seq, names, name_off, max_win, status."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

OK, IRREGULAR, OVERFLOW = 0, 1, 2
Parsed = namedtuple("Parsed", "verdict offence records")


def lines_of(data: bytes):
    """[(start, end)] of every line: end is the position of its '\\n', or len(data)"""
    out, p, n = [], 0, len(data)
    while p < n:
        e = data.find(b"\n", p)
        if e < 0:
            e = n
        out.append((p, e))
        p = e + 1
    return out


def trimmed_end(data: bytes, b: int, e: int) -> int:
    while e > b and data[e - 1] in b"\r\n":
        e -= 1
    return e


def parse(data: bytes) -> Parsed:
    data = bytes(data)
    if not data or data[0] not in b">@":
        return Parsed(IRREGULAR, 0, [])
    fastq = data[0:1] == b"@"
    lines = lines_of(data)
    recs, offence = [], None

    def offend(p):
        nonlocal offence
        if offence is None or p < offence:
            offence = p

    if fastq:
        for k, (b, e) in enumerate(lines):
            c = data[b:b + 1]                                   # (the '\n' itself for an empty line)
            ph = k & 3
            if ph == 0 and c != b"@":
                offend(b)
            if ph == 1 and c in (b"+", b">", b"\n", b"\r"):
                offend(b)
            if ph == 2 and c != b"+":
                offend(b)
        if len(lines) & 3:
            offend(len(data))
        if offence is None:
            for k in range(0, len(lines), 4):
                hb, he = lines[k]
                sb, se = lines[k + 1]
                recs.append((hb + 1, trimmed_end(data, hb + 1, he) - (hb + 1), data[sb:trimmed_end(data, sb, se)]))
    else:
        cur = None
        for b, e in lines:
            c = data[b:b + 1]
            if c == b"+":
                offend(b)
            if c == b">":
                if cur:
                    recs.append((cur[0], cur[1], b"".join(cur[2])))
                cur = (b + 1, trimmed_end(data, b + 1, e) - (b + 1), [])
            else:
                cur[2].append(data[b:trimmed_end(data, b, e)])
        recs.append((cur[0], cur[1], b"".join(cur[2])))
    if offence is not None:
        return Parsed(IRREGULAR, offence, [])
    return Parsed(OK, 0, recs)


def name_of(data: bytes, hdr_off: int, hdr_len: int) -> bytes:
    h = bytes(data[hdr_off:hdr_off + hdr_len])
    k = h.find(b" ")
    return h if k < 0 else h[:k]


def reads_of(parsed: Parsed, pairs: bool = False):
    """-> (reads, mates or None) as Database.query takes them; an odd record count leaves a last mate b'' """
    seqs = [r[2] for r in parsed.records]
    if not pairs:
        return seqs, None
    return seqs[0::2], [seqs[k + 1] if k + 1 < len(seqs) else b"" for k in range(0, len(seqs), 2)]


def pack(data: bytes, parsed: Parsed, *, pairs: bool = False, insert_max: int = 0, stride: int = 1):
    """what mc_parse_records writes for an accepted range -> dict(hdr, qinfo, seq, names, name_off, max_win, status)"""
    recs = parsed.records
    per = 2 if pairs else 1
    nq = (len(recs) + per - 1) // per
    hdr = np.array([[r[0], r[1]] for r in recs], dtype=np.uint32).reshape(len(recs), 2)
    qinfo = np.zeros((nq, 4), dtype=np.uint32)
    max_win = np.zeros(nq, dtype=np.uint32)
    seq = bytearray()
    names, name_off = bytearray(), np.zeros(nq + 1, dtype=np.uint64)
    longest = 0
    for q in range(nq):
        mates = recs[q * per:(q + 1) * per]
        for m in range(2):
            s = mates[m][2] if m < len(mates) else b""
            qinfo[q, 2 * m], qinfo[q, 2 * m + 1] = len(seq), len(s)
            seq += s + b"\0" * (-len(s) % 4)
        both = int(qinfo[q, 1]) + int(qinfo[q, 3])
        longest = max(longest, both)
        max_win[q] = 2 + max(both, insert_max) // stride
        names += name_of(data, mates[0][0], mates[0][1])
        name_off[q + 1] = len(names)
    seq += b"\0" * 16
    status = np.array([len(recs), nq, len(seq), len(names), OK, 0, longest, 1 if pairs and len(recs) & 1 else 0], dtype=np.uint64)
    return dict(hdr=hdr, qinfo=qinfo, seq=bytes(seq), names=bytes(names), name_off=name_off, max_win=max_win, status=status)
