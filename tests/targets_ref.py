"""The target rule of mc_parse_targets (include/metacache_amd.h) in plain Python: the model the device parse is held to.

The range is the files back to back; file f is data[file_off[f]:file_off[f + 1]].  Each file is judged by parse_ref.parse on its own, plus
what the device refuses beyond the record rule: a first byte that is not '>' (FASTQ is not taken) and a '\\r' that is not followed by '\\n'
or by the file's end.  The lowest offence of the range wins.  A file table that breaks its own rule (row 0 is 0, every row lies above the
one in front of it, the last row is the range's length) gives IRREGULAR with the offence len(data) and the first bad row.
parse(files) / parse_range(data, file_off) -> Parsed(verdict, offence, file, records), records = [(hdr_off, hdr_len, seq, file, index)] with
hdr_off in the range.  pack(parsed) lays targets, seq and status out as the call does."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import parse_ref

OK, IRREGULAR, OVERFLOW = parse_ref.OK, parse_ref.IRREGULAR, parse_ref.OVERFLOW
Parsed = namedtuple("Parsed", "verdict offence file records")
target_dtype = np.dtype([("seq_off", "<u8"), ("len", "<u4"), ("file", "<u4"), ("index", "<u4"), ("reserved", "<u4")])
assert target_dtype.itemsize == 24


def table_of(files):
    """file_off [len(files) + 1] of files laid back to back"""
    off = np.zeros(len(files) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(f) for f in files], dtype=np.uint64)
    return off


def first_bad_row(file_off, nbytes):
    """the first row that breaks the table's rule, or None"""
    off = [int(x) for x in file_off]
    for r, o in enumerate(off):
        if (r == 0 and o != 0) or (r > 0 and o <= off[r - 1]) or (r == len(off) - 1 and o != nbytes):
            return r
    return None


def lone_cr(data: bytes):
    """the first '\\r' of a file that is followed neither by '\\n' nor by the file's end, or None"""
    p = data.find(b"\r")
    while p >= 0:
        if p + 1 < len(data) and data[p + 1:p + 2] != b"\n":
            return p
        p = data.find(b"\r", p + 1)
    return None


def parse_file(data: bytes):
    """one file on its own -> (offence or None, records of parse_ref)"""
    if data[0:1] != b">":
        return 0, []
    got = parse_ref.parse(data)
    offences = [got.offence] if got.verdict != OK else []
    cr = lone_cr(data)
    if cr is not None:
        offences.append(cr)
    if offences:
        return min(offences), []
    return None, got.records


def parse_range(data: bytes, file_off) -> Parsed:
    data = bytes(data)
    bad = first_bad_row(file_off, len(data))
    if bad is not None:
        return Parsed(IRREGULAR, len(data), bad, [])
    off = [int(x) for x in file_off]
    records = []
    for f in range(len(off) - 1):
        offence, recs = parse_file(data[off[f]:off[f + 1]])
        if offence is not None:                                 # (files in order: the first file with an offence holds the lowest one)
            return Parsed(IRREGULAR, off[f] + offence, f, [])
        records += [(off[f] + h, hl, s, f, i) for i, (h, hl, s) in enumerate(recs)]
    return Parsed(OK, 0, 0, records)


def parse(files) -> Parsed:
    return parse_range(b"".join(files), table_of(files))


def pack(parsed: Parsed):
    """what mc_parse_targets writes -> dict(hdr, targets, seq, status); with IRREGULAR only status"""
    if parsed.verdict != OK:
        return dict(status=np.array([0, 0, 0, 0, parsed.verdict, parsed.offence, 0, parsed.file], dtype=np.uint64))
    recs = parsed.records
    hdr = np.array([[r[0], r[1]] for r in recs], dtype=np.uint32).reshape(len(recs), 2)
    targets = np.zeros(len(recs), dtype=target_dtype)
    seq = bytearray()
    for k, (_, _, s, f, i) in enumerate(recs):
        targets[k] = (len(seq), len(s), f, i, 0)
        seq += s + b"\0" * (-len(s) % 4)
    seq += b"\0" * 16
    status = np.array([len(recs), sum(1 for r in recs if r[2]), len(seq), 0, OK, 0, max((len(r[2]) for r in recs), default=0), 0], dtype=np.uint64)
    return dict(hdr=hdr, targets=targets, seq=bytes(seq), status=status)


def headers_of(data: bytes, parsed: Parsed):
    return [bytes(data[r[0]:r[0] + r[1]]) for r in parsed.records]
