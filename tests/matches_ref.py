"""Plain Python model of mc_format_matches and of the extra column of mc_format_mappings_with (include/metacache_amd.h, "the all-hits
column"): a read's location list, run-length encoded, and the mapping line that carries it.

Written from the rule, one read at a time; the tests compare the device against it (test_gpu_matches.py), and it against the
reference's own output lines (test_matches_witness_cpu.py)."""
from __future__ import annotations

import numpy as np

import format_ref

WINDOWS = 2                              # MC_MATCHES_WINDOWS


def runs_of(hits):
    """hits: an array with fields win, tgt -> [(tgt, win, length)]: maximal stretches of consecutive equal entries, in list order"""
    if len(hits) == 0:
        return []
    tgt, win = np.asarray(hits["tgt"], dtype=np.int64), np.asarray(hits["win"], dtype=np.int64)
    heads = np.concatenate([[0], np.flatnonzero((tgt[1:] != tgt[:-1]) | (win[1:] != win[:-1])) + 1])
    ends = np.concatenate([heads[1:], [len(tgt)]])
    return [(int(tgt[h]), int(win[h]), int(e - h)) for h, e in zip(heads, ends)]


def piece(hits, texts, windows: bool, tally=None) -> bytes:
    """one read's column.  texts: list of bytes per target.  tally: [runs printed, runs whose target lay beyond the table], added to"""
    tally = tally if tally is not None else [0, 0]
    out = bytearray()
    for tgt, win, length in runs_of(hits):
        if tgt >= len(texts):
            tally[1] += 1                                      # prints nothing, in both forms
            continue
        t = texts[tgt]
        if windows:
            if not t:
                continue                                       # the host's `if (t)`: a target without a taxon prints nothing at all
            signed = win - (1 << 32) if win >= (1 << 31) else win                  # int(win)
            out += t + b"/" + str(signed).encode() + b":" + str(length).encode() + b","
        else:
            out += t + b":" + str(length).encode() + b","
        tally[0] += 1
    return bytes(out)


def format_all(hits: np.ndarray, hit_off, texts, windows: bool):
    """-> (all bytes, piece_off uint64 [n + 1], runs printed, runs beyond the table)"""
    n = len(hit_off) - 1
    tally = [0, 0]
    chunks, off, at = [], np.zeros(n + 1, dtype=np.uint64), 0
    for i in range(n):
        p = piece(hits[int(hit_off[i]):int(hit_off[i + 1])], texts, windows, tally)
        chunks.append(p)
        at += len(p)
        off[i + 1] = at
    return b"".join(chunks), off, tally[0], tally[1]


def line(i: int, *, extra, column: bytes, flags: int, cands, taxon: int, rank: int, name: bytes, result, target_result=None, cand_text=(),
         truth: int = 0, query_id: int = 0, win_stride: int = 0, win_len: int = 0, beyond=None) -> bytes:
    """format_ref.line with one more column between the truth column and the tophits column: `extra` (bytes) and the separator.
    extra None: format_ref.line itself.  A read without a line (MAPPED_ONLY, unclassified) has none here either: its piece is skipped."""
    if extra is None:
        return format_ref.line(i, column=column, flags=flags, cands=cands, taxon=taxon, rank=rank, name=name, result=result, target_result=target_result,
                               cand_text=cand_text, truth=truth, query_id=query_id, win_stride=win_stride, win_len=win_len, beyond=beyond)
    beyond = beyond if beyond is not None else [0]
    if (flags & format_ref.MAPPED_ONLY) and taxon == 0:
        return b""
    used = []
    for c in cands:
        if int(c["hits"]) == 0:
            break
        used.append((int(c["tgt"]), int(c["hits"]), int(c["beg"]), int(c["end"])))
    out = bytearray()
    if flags & format_ref.QUERY_IDS:
        out += str(query_id & format_ref.U64).encode() + column
    out += name + column
    if flags & format_ref.TRUTH:
        out += format_ref.result_text(result, truth, beyond) + column
    out += bytes(extra) + column                                   # where MappingWriter prints -allhits
    if flags & format_ref.TOPHITS:
        parts = []
        for tgt, hits, _, _ in used:
            t = cand_text[tgt] if tgt < len(cand_text) else b""
            parts.append(t + b":" + str(hits).encode() if t else b"")
        out += b",".join(parts) + column
    if flags & format_ref.LOCATIONS:
        for _, _, beg, end in used:
            out += b"[" + str(win_stride * beg).encode() + b"," + str(win_stride * end + win_len).encode() + b"] "
        out += column
    if taxon != 0 and rank == 0 and target_result and len(cands):
        tgt = int(cands[0]["tgt"])
        out += target_result[tgt] if tgt < len(target_result) else format_ref.result_text(result, len(result), beyond)
    else:
        out += format_ref.result_text(result, taxon, beyond)
    out += b"\n"
    return bytes(out)


def lines_all(*, extra, extra_off, column: bytes, flags: int, cands: np.ndarray, assigned: np.ndarray, names, result, target_result=None, cand_text=(),
              truth=None, query_ids=None, first_query_id: int = 0, win_stride: int = 0, win_len: int = 0):
    """format_ref.format_all with the extra column: piece i = extra[extra_off[i] .. extra_off[i + 1]) -> (all bytes, line_off, lines, beyond)"""
    n = len(assigned)
    beyond = [0]
    chunks, off, lines, at = [], np.zeros(n + 1, dtype=np.uint64), 0, 0
    for i in range(n):
        l = line(i, extra=extra[int(extra_off[i]):int(extra_off[i + 1])], column=column, flags=flags, cands=cands[i], taxon=int(assigned["taxon"][i]),
                 rank=int(assigned["rank"][i]), name=bytes(names[i]), result=result, target_result=target_result, cand_text=cand_text,
                 truth=int(truth[i]) if truth is not None else 0, query_id=int(query_ids[i]) if query_ids is not None else first_query_id + i,
                 win_stride=win_stride, win_len=win_len, beyond=beyond)
        chunks.append(l)
        lines += 1 if l else 0
        at += len(l)
        off[i + 1] = at
    return b"".join(chunks), off, lines, beyond[0]
