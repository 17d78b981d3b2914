"""Plain numpy model of the per-target hit lists (include/metacache_amd.h, "per-target hit lists"): what mc_target_hits_add /
mc_target_hits_collect must compute.  Written from the rules of the header: which entries qualify is classify_ref's tax rule (the one
of mc_coverage_add), the order is one np.lexsort over the five fields, the slices come from np.searchsorted."""
from __future__ import annotations

import numpy as np

import classify_ref

NUM_RANKS = classify_ref.NUM_RANKS
hit_dtype = np.dtype([("tgt", "<u4"), ("beg", "<u4"), ("end", "<u4"), ("hits", "<u4"), ("query", "<u8")])


def tax(lin: np.ndarray, tgt: int, lowest: int) -> int:
    """tax(c) as the vote takes it for its top candidate (classify_ref.vote): lineage slot `lowest` itself for rank 0, else the first
    non-zero slot from `lowest` up; a tgt beyond the table has the lineage of zeros"""
    row = classify_ref.lineage_of(lin, int(tgt))
    if lowest == 0:
        return int(row[0])
    return next((int(row[k]) for k in range(lowest, NUM_RANKS) if row[k] != 0), 0)


def tax_all(lin: np.ndarray, tgt: np.ndarray, lowest: int) -> np.ndarray:
    """tax() for arrays of targets, every step for all entries at once (checked against tax() by the CPU tests)"""
    nt = len(lin)
    linx = np.vstack([lin.astype(np.int64), np.zeros((1, NUM_RANKS), dtype=np.int64)])
    rows = linx[np.where(tgt < nt, tgt, nt).astype(np.int64)]
    if lowest == 0:
        return rows[..., 0]
    up = rows[..., lowest:]
    first = (up != 0).argmax(axis=-1)
    return np.take_along_axis(up, first[..., None], axis=-1)[..., 0]


def records_of(lin: np.ndarray, cands: np.ndarray, hits_min: int, lowest: int, query_ids=None, first_query_id: int = 0) -> np.ndarray:
    """the records of cands[n, stride], in row order (unsorted)"""
    n, stride = cands.shape
    used = np.cumsum(cands["hits"] == 0, axis=1) == 0                               # the entries in front of a row's first hits == 0
    q = used & (cands["hits"].astype(np.int64) >= hits_min) & (tax_all(lin, cands["tgt"].astype(np.int64), lowest) != 0)
    ids = (np.uint64(first_query_id) + np.arange(n, dtype=np.uint64)) if query_ids is None else np.asarray(query_ids, dtype=np.uint64)
    out = np.zeros(int(q.sum()), dtype=hit_dtype)
    for f in ("tgt", "beg", "end", "hits"):
        out[f] = cands[f][q]
    out["query"] = np.broadcast_to(ids[:, None], (n, stride))[q]
    return out


def sort_records(rec: np.ndarray) -> np.ndarray:
    """ascending by (tgt, beg, end, query, hits), query as a 64-bit number"""
    return rec[np.lexsort((rec["hits"], rec["query"], rec["end"], rec["beg"], rec["tgt"]))]


def collect(rec: np.ndarray, num_targets: int):
    """-> (offsets[num_targets + 1] uint64, sorted records, targets with at least one record)"""
    s = sort_records(rec)
    offsets = np.searchsorted(s["tgt"], np.arange(num_targets + 1), side="left").astype(np.uint64)
    return offsets, s, int((np.diff(offsets.astype(np.int64)) > 0).sum())
