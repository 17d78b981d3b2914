"""The mates rule of mc_parse_mates (include/metacache_amd.h) in plain Python, on top of parse_ref.parse.

Two ranges B1 and B2, each judged by the record rule on its own; query q is record q of B1 (first mate, the name) and record q of B2.
mates(data1, data2, ...) -> dict(status [10]) and, with the verdict OK, hdr [2 * queries, 2] (row 2q in B1, row 2q + 1 in B2), qinfo,
seq, names, name_off, max_win laid out as mc_parse_records(MC_PARSE_PAIRS) lays out a file in which the records alternate.
interleave(data1, data2) builds such a file (FASTA) from the two ranges' records, for the cross-check against parse_ref.pack."""
from __future__ import annotations

import numpy as np

import parse_ref

OK, IRREGULAR, OVERFLOW, UNEQUAL = 0, 1, 2, 3


def mates(data1: bytes, data2: bytes, *, insert_max: int = 0, stride: int = 1, max_records=None, seq_capacity=None, names_capacity=None):
    data = (bytes(data1), bytes(data2))
    parsed = [parse_ref.parse(d) for d in data]
    status = np.zeros(10, dtype=np.uint64)
    for f in range(2):                                           # range 0's offence goes first
        if parsed[f].verdict != parse_ref.OK:
            status[4], status[5], status[7] = IRREGULAR, parsed[f].offence, f
            return dict(status=status)
    r1, r2 = len(parsed[0].records), len(parsed[1].records)
    status[0], status[8], status[9] = r1 + r2, r1, r2
    if r1 != r2:
        status[1], status[4] = min(r1, r2), UNEQUAL
        return dict(status=status)
    nq = r1
    hdr = np.zeros((2 * nq, 2), dtype=np.uint32)
    qinfo = np.zeros((nq, 4), dtype=np.uint32)
    max_win = np.zeros(nq, dtype=np.uint32)
    name_off = np.zeros(nq + 1, dtype=np.uint64)
    seq, names, longest = bytearray(), bytearray(), 0
    for q in range(nq):
        for f in range(2):
            off, length, s = parsed[f].records[q]
            hdr[2 * q + f] = (off, length)
            qinfo[q, 2 * f], qinfo[q, 2 * f + 1] = len(seq), len(s)
            seq += s + b"\0" * (-len(s) % 4)
        both = int(qinfo[q, 1]) + int(qinfo[q, 3])
        longest = max(longest, both)
        max_win[q] = 2 + max(both, insert_max) // stride
        names += parse_ref.name_of(data[0], *parsed[0].records[q][:2])
        name_off[q + 1] = len(names)
    seq += b"\0" * 16
    status[1], status[2], status[3] = nq, len(seq), len(names)
    fits = max_records is None or 2 * nq <= max_records
    status[6] = longest if fits else 0                           # (the per-record tables hold max_records records: no longest without them)
    if not fits or (seq_capacity is not None and len(seq) > seq_capacity) or (names_capacity is not None and len(names) > names_capacity):
        status[4] = OVERFLOW
        return dict(status=status)
    return dict(status=status, hdr=hdr, qinfo=qinfo, seq=bytes(seq), names=bytes(names), name_off=name_off, max_win=max_win)


def interleave(data1: bytes, data2: bytes) -> bytes:
    """a FASTA file in which the records of the two (accepted, equally long) ranges alternate: each header as it stood, each sequence on one line"""
    data = (bytes(data1), bytes(data2))
    parsed = [parse_ref.parse(d) for d in data]
    assert all(p.verdict == parse_ref.OK for p in parsed) and len(parsed[0].records) == len(parsed[1].records)
    out = bytearray()
    for q in range(len(parsed[0].records)):
        for f in range(2):
            off, length, s = parsed[f].records[q]
            out += b">" + data[f][off:off + length] + b"\n" + s + b"\n"
    return bytes(out)
