"""Plain model of `query -align`: the semi-global alignment (match +2, mismatch -1, gap -1, free end gaps; ties fall to diag, then
above, then left; end cell = the corner unless a cell of the last column, then of the last row, is strictly greater; the trace is a
do-while, so an empty side gives one column of gaps), the choice between read 1 forward and reverse-complemented (the mate's two
scores added as unsigned 64-bit numbers; forward only when strictly greater), the cut of the subject out of the target's record and
the three output lines.

ONE parameter, the record rule: the database stores a target's record number in its file 0-based; the reference program reads
record `index - 1` ("reference": the record before the target, none for a file's first record), mcq reads record `index` ("mcq").
Rows are numpy vectors: the left-gap dependency along a row is a running maximum of (value + column) - column."""
from __future__ import annotations

import gzip
import os

import numpy as np

MASK64 = (1 << 64) - 1
_COMP = bytes.maketrans(b"AaCcGgTtUu", b"TtGgCcAaAa")


def reverse_complement(s: bytes) -> bytes:
    return s[::-1].translate(_COMP)


def semiglobal(q: bytes, s: bytes, trace: bool = True):
    """-> (score, aligned query, aligned subject) (the strings are None without trace)"""
    lq, ls = len(q), len(s)
    if lq == 0 or ls == 0:
        return 0, (b"_" if trace else None), (b"_" if trace else None)
    sa = np.frombuffer(s, dtype=np.uint8)
    idx = np.arange(ls + 1, dtype=np.int64)
    prev = np.zeros(ls + 1, dtype=np.int64)
    pred = np.zeros((lq + 1, ls + 1), dtype=np.uint8) if trace else None
    lastcol = np.zeros(lq + 1, dtype=np.int64)
    for i in range(1, lq + 1):
        d = prev[:-1] + np.where(sa == q[i - 1], 2, -1)
        a = prev[1:] - 1
        t = np.empty(ls + 1, dtype=np.int64)
        t[0] = 0
        np.maximum(d, a, out=t[1:])
        cur = np.maximum.accumulate(t + idx) - idx             # cur[j] = max(t[j], cur[j-1] - 1)
        if trace:
            p = np.where(a > d, 2, 1).astype(np.uint8)
            p[cur[1:] > t[1:]] = 3
            pred[i, 1:] = p
        lastcol[i] = cur[ls]
        prev = cur
    bq, bs, bv = lq, ls, int(prev[ls])
    if lq > 1:
        k = int(np.argmax(lastcol[1:lq])) + 1                  # first of the greatest, rows 1 .. lq-1
        if lastcol[k] > bv:
            bq, bs, bv = k, ls, int(lastcol[k])
    if ls > 1:
        k = int(np.argmax(prev[1:ls])) + 1
        if prev[k] > bv:
            bq, bs, bv = lq, k, int(prev[k])
    if not trace:
        return bv, None, None
    aq, at = bytearray(), bytearray()
    while True:
        p = pred[bq, bs]
        if p == 1:
            bq -= 1; bs -= 1; aq.append(q[bq]); at.append(s[bs])
        elif p == 2:
            bq -= 1; aq.append(q[bq]); at.append(95)
        elif p == 3:
            bs -= 1; aq.append(95); at.append(s[bs])
        else:
            aq.append(95); at.append(95)
        if pred[bq, bs] == 0:
            break
    return bv, bytes(aq[::-1]), bytes(at[::-1])


def align_pair(read: bytes, mate: bytes | None, subject: bytes):
    """-> (score, reversed, aligned query, aligned subject, [read forward, reverse, mate forward, reverse])"""
    f, fq, ft = semiglobal(read, subject)
    r, rq, rt = semiglobal(reverse_complement(read), subject)
    mf = mr = 0
    if mate:
        mf = semiglobal(mate, subject, trace=False)[0]
        mr = semiglobal(reverse_complement(mate), subject, trace=False)[0]
    forward = ((f + mf) & MASK64) > ((r + mr) & MASK64)
    return (f, False, fq, ft, [f, r, mf, mr]) if forward else (r, True, rq, rt, [f, r, mf, mr])


# ---- sequence files ---------------------------------------------------------------------------------------------------------------
def read_records(path: str):
    """[(header, sequence)] of a FASTA / FASTQ file (gzip by name), lines joined, characters as they are"""
    op = gzip.open if path.endswith(".gz") else open
    with op(path, "rb") as f:
        lines = f.read().split(b"\n")
    recs, i = [], 0
    while i < len(lines) and not lines[i][:1] in (b">", b"@"):
        i += 1
    while i < len(lines):
        ln = lines[i].rstrip(b"\r")
        if ln[:1] == b">":
            h = ln[1:]; i += 1; seq = []
            while i < len(lines) and lines[i][:1] != b">":
                seq.append(lines[i].rstrip(b"\r")); i += 1
            recs.append((h, b"".join(seq)))
        elif ln[:1] == b"@":
            recs.append((ln[1:], lines[i + 1].rstrip(b"\r") if i + 1 < len(lines) else b"")); i += 4
        else:
            i += 1
    return recs


class Records:
    """target records by (file name, number), files read once; a missing file or record: None"""

    def __init__(self, base: str):
        self.base, self.files = base, {}

    def get(self, filename: str, number: int):
        if filename not in self.files:
            p = os.path.join(self.base, filename)
            self.files[filename] = read_records(p) if os.path.isfile(p) else None
        recs = self.files[filename]
        if recs is None or number < 0 or number >= len(recs):
            return None
        return recs[number][1]


def record_number(index: int, rule: str) -> int:
    """which record of the source file is read for a target whose stored record number is `index`"""
    if rule == "reference":
        return index - 1            # sequence_reader::skip(index - 1): index 0 skips past the end of the file -> -1 = none
    if rule == "mcq":
        return index
    raise ValueError(rule)


def cut(record: bytes, beg: int, end: int, winlen: int, stride: int) -> bytes:
    """make_view_from_window_range: windows beg .. end of the record"""
    return record[stride * beg:min(stride * end + winlen, len(record))]


def alignment_lines(records: Records, rule: str, comment: str, filename: str, index: int, beg: int, end: int, winlen: int, stride: int,
                    read: bytes, mate: bytes | None):
    """the three lines that follow a mapping line's taxon text (without the '\\n' before the first), or None where none are printed"""
    rec = records.get(filename, record_number(index, rule))
    if rec is None:
        return None
    score, _, aq, at, _ = align_pair(read, mate, cut(rec, beg, end, winlen, stride))
    return [f"{comment}  score  {score}  aligned to {filename} #{index} in range [{stride * beg},{stride * end + stride}]",
            f"{comment}  query  {aq.decode('latin-1')}", f"{comment}  target {at.decode('latin-1')}"]


# ---- output files of `query -align` -----------------------------------------------------------------------------------------------
import re

SKETCHING = {"default": (127, 112), "w64": (64, 40)}            # database of the goldens -> (winlen, winstride)
_HEAD = re.compile(r"^  score  (-?\d+)  aligned to (.+) #(\d+) in range \[(\d+),(\d+)\]$")


def option(args, name, default):
    return args[args.index(name) + 1] if name in args else default


def parse_output(lines, comment):
    """-> [(number of the mapping line, mapping line, its three alignment lines or None)]"""
    out, i = [], 0
    while i < len(lines):
        ln = lines[i]
        if ln == "" or ln.startswith(comment):
            i += 1
            continue
        if i + 3 < len(lines) + 1 and i + 1 < len(lines) and lines[i + 1].startswith(comment + "  score  "):
            out.append((i, ln, lines[i + 1:i + 4])); i += 4
        else:
            out.append((i, ln, None)); i += 1
    return out


def parse_head(line, comment, stride):
    """first alignment line -> (score, file name, record number as printed, first window, last window)"""
    m = _HEAD.match(line[len(comment):])
    assert m, line
    return int(m.group(1)), m.group(2), int(m.group(3)), int(m.group(4)) // stride, int(m.group(5)) // stride - 1


def columns(lines, comment, sep):
    """names of the mapping lines' columns, from the TABLE_LAYOUT line"""
    for ln in lines:
        if ln.startswith(comment + "TABLE_LAYOUT: "):
            return [c.strip() for c in ln[len(comment) + 14:].split(sep)]
    raise AssertionError("no TABLE_LAYOUT line")


def queries(path, paired):
    """read name (first word of the header) -> (read, mate or None)"""
    recs = read_records(path)
    if paired:
        return {recs[i][0].split(b" ")[0].decode(): (recs[i][1], recs[i + 1][1]) for i in range(0, len(recs) - 1, 2)}
    return {h.split(b" ")[0].decode(): (s, None) for h, s in recs}


def first_record_names(base, files):
    """sequence ids (first word of the header) of the records that open a file"""
    return {read_records(os.path.join(base, f))[0][0].split(b" ")[0].decode() for f in files}
