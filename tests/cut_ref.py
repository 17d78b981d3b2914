"""The cut rule of mc_parse_cut (include/metacache_amd.h) in plain Python, on top of parse_ref.lines_of: the model the device
cut is held to.

cut(data, R, pairs=False, open=False) -> Cut(verdict, offence, whole, consumed, cuts, seen, longest, half).  Line starts, record starts
and offences are those of the record rule (parse_ref); the rule adds where the range is taken to end.  cuts is [] with a verdict other
than OK (capacity is the caller's affair: the model never overflows), longest then 0.  headers(data, parsed) is what mc_parse_headers
packs: (bytes, offsets)."""
from __future__ import annotations

from collections import namedtuple

import parse_ref
from parse_ref import IRREGULAR, OK

Cut = namedtuple("Cut", "verdict offence whole consumed cuts seen longest half")


def offences_of(data: bytes, lines, fastq: bool):
    """every position that breaks the record rule inside the range, in order (without the incomplete last group)"""
    out = []
    for k, (b, e) in enumerate(lines):
        c = data[b:b + 1]
        if fastq:
            ph = k & 3
            if (ph == 0 and c != b"@") or (ph == 1 and c in (b"+", b">", b"\n", b"\r")) or (ph == 2 and c != b"+"):
                out.append(b)
        elif c == b"+":
            out.append(b)
    n, p = len(data), data.find(b"\r")
    while p >= 0:                                                  # a '\r' that is followed neither by '\n' nor by the end of the range
        if p + 1 < n and data[p + 1] != 10:
            out.append(p)
        p = data.find(b"\r", p + 1)
    return sorted(out)


def cut(data: bytes, R: int, pairs: bool = False, open: bool = False) -> Cut:
    data = bytes(data)
    n = len(data)
    assert n > 0 and R > 0 and not (pairs and R & 1)
    fastq = data[0:1] == b"@"
    lines = parse_ref.lines_of(data)
    starts = [b for k, (b, e) in enumerate(lines) if (k & 3) == 0] if fastq else [b for b, e in lines if data[b:b + 1] == b">"]
    seen = len(starts)
    if not open:
        whole, consumed = seen, n
    else:
        whole = data.count(b"\n") // 4 if fastq else max(seen, 1) - 1
        if pairs:
            whole &= ~1
        consumed = starts[whole] if whole < seen else (n if seen else 0)
    offs = [o for o in offences_of(data, lines, fastq) if o < consumed]
    if not open and fastq and len(lines) & 3:
        offs.append(n)
    if data[0:1] not in (b">", b"@"):
        offs = [0]
    if offs:
        return Cut(IRREGULAR, min(offs), whole, consumed, [], seen, 0, 0)
    cuts = [starts[k] for k in range(0, whole, R)] + [consumed]
    longest = max((b - a for a, b in zip(cuts, cuts[1:])), default=0)
    return Cut(OK, 0, whole, consumed, cuts, seen, longest, 1 if (not open and pairs and whole & 1) else 0)


def status_of(c: Cut):
    """the eight words of mc_parse_cut's status"""
    nb = max(len(c.cuts) - 1, 0) if c.verdict == OK else None
    return [c.whole, nb, c.consumed, c.seen, c.verdict, c.offence, c.longest, c.half]


def headers(data: bytes, parsed: parse_ref.Parsed):
    """-> (the trimmed headers back to back, [offset of each, and the end])"""
    out, off = bytearray(), [0]
    for h_off, h_len, _ in parsed.records:
        out += data[h_off:h_off + h_len]
        off.append(len(out))
    return bytes(out), off
