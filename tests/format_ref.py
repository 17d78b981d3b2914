"""Plain Python model of mc_format_mappings (include/metacache_amd.h, "mapping lines"): the bytes of every read's line, from the same
arrays and string tables the library is given.

Written from the rule, one read at a time; the tests compare the device against it (test_gpu_format.py), and it against the
reference's own output lines (test_format_witness_cpu.py)."""
from __future__ import annotations

import numpy as np

QUERY_IDS, TRUTH, TOPHITS, LOCATIONS, MAPPED_ONLY = 2, 4, 8, 16, 32
U64 = (1 << 64) - 1


def result_text(result, taxon: int, beyond: list) -> bytes:
    """entry `taxon` of the result table; an index beyond it takes entry 0 and is counted"""
    if taxon >= len(result):
        beyond[0] += 1
        taxon = 0
    return result[taxon]


def line(i: int, *, column: bytes, flags: int, cands, taxon: int, rank: int, name: bytes, result, target_result=None, cand_text=(),
         truth: int = 0, query_id: int = 0, win_stride: int = 0, win_len: int = 0, beyond=None) -> bytes:
    """one read: cands = its row (fields tgt, hits, beg, end), taxon / rank = its assignment.  b"" = no line"""
    beyond = beyond if beyond is not None else [0]
    if (flags & MAPPED_ONLY) and taxon == 0:
        return b""
    used = []
    for c in cands:
        if int(c["hits"]) == 0:
            break
        used.append((int(c["tgt"]), int(c["hits"]), int(c["beg"]), int(c["end"])))
    out = bytearray()
    if flags & QUERY_IDS:
        out += str(query_id & U64).encode() + column
    out += name + column
    if flags & TRUTH:
        out += result_text(result, truth, beyond) + column
    if flags & TOPHITS:
        parts = []
        for tgt, hits, _, _ in used:
            t = cand_text[tgt] if tgt < len(cand_text) else b""
            parts.append(t + b":" + str(hits).encode() if t else b"")
        out += b",".join(parts) + column
    if flags & LOCATIONS:
        for _, _, beg, end in used:
            out += b"[" + str(win_stride * beg).encode() + b"," + str(win_stride * end + win_len).encode() + b"] "
        out += column
    if taxon != 0 and rank == 0 and target_result and len(cands):
        tgt = int(cands[0]["tgt"])
        out += target_result[tgt] if tgt < len(target_result) else result_text(result, len(result), beyond)
    else:
        out += result_text(result, taxon, beyond)
    out += b"\n"
    return bytes(out)


def format_all(*, column: bytes, flags: int, cands: np.ndarray, assigned: np.ndarray, names, result, target_result=None, cand_text=(),
               truth=None, query_ids=None, first_query_id: int = 0, win_stride: int = 0, win_len: int = 0):
    """cands[n, stride], assigned[n] (fields taxon, rank), names: n bytes -> (all bytes, line_off uint64 [n + 1], lines, beyond)"""
    n = len(assigned)
    beyond = [0]
    chunks, off, lines = [], np.zeros(n + 1, dtype=np.uint64), 0
    at = 0
    for i in range(n):
        l = line(i, column=column, flags=flags, cands=cands[i], taxon=int(assigned["taxon"][i]), rank=int(assigned["rank"][i]), name=bytes(names[i]),
                 result=result, target_result=target_result, cand_text=cand_text, truth=int(truth[i]) if truth is not None else 0,
                 query_id=int(query_ids[i]) if query_ids is not None else first_query_id + i, win_stride=win_stride, win_len=win_len, beyond=beyond)
        chunks.append(l)
        lines += 1 if l else 0
        at += len(l)
        off[i + 1] = at
    return b"".join(chunks), off, lines, beyond[0]
