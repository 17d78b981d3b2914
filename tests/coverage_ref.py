"""Plain numpy model of the target coverage calls (include/metacache_amd.h, "target coverage"): what mc_coverage_add / _counts,
mc_coverage_keep and mc_coverage_drop must compute.  Written from the rules of the header, not from the kernels: marking is a difference
array over all windows of all targets, the percentile filter is sequential numpy.float32 arithmetic, one operation at a time."""
from __future__ import annotations

import numpy as np

NUM_RANKS = 21


def used(cands: np.ndarray) -> np.ndarray:
    """[n, stride] bool: the entries in front of a row's first hits == 0"""
    return np.cumsum(cands["hits"] == 0, axis=1) == 0


def tax(lin: np.ndarray, tgt: np.ndarray, lowest: int) -> np.ndarray:
    """tax(c) per entry: lineage slot `lowest` itself for rank 0, else the first non-zero slot from `lowest` up; 0 for a tgt beyond the table"""
    nt = len(lin)
    linx = np.vstack([lin.astype(np.int64), np.zeros((1, NUM_RANKS), dtype=np.int64)])
    rows = linx[np.where(tgt < nt, tgt, nt).astype(np.int64)]                       # [..., 21]
    if lowest == 0:
        return rows[..., 0]
    up = rows[..., lowest:]
    first = (up != 0).argmax(axis=-1)
    return np.take_along_axis(up, first[..., None], axis=-1)[..., 0]                # (0 where every slot is 0)


def mark(windows: np.ndarray, lin: np.ndarray, cands: np.ndarray, hits_min: int, lowest: int):
    """-> (covered[targets] uint32, out-of-range entries, entries that marked windows)"""
    windows = np.asarray(windows, dtype=np.int64)
    nt = len(windows)
    tgt, hits = cands["tgt"].astype(np.int64), cands["hits"].astype(np.int64)
    beg, end = cands["beg"].astype(np.int64), cands["end"].astype(np.int64)
    q = used(cands) & (hits >= hits_min) & (tax(lin, tgt, lowest) != 0)             # qualifying entries
    tgt, beg, end = tgt[q], beg[q], end[q]
    win = windows[np.where(tgt < nt, tgt, 0)]
    nothing = (tgt >= nt) | (beg > end) | (beg >= win)                              # marks nothing
    clipped = ~nothing & (end >= win)                                               # marks its in-range part
    out_of_range = int(nothing.sum() + clipped.sum())
    tgt, beg, end, win = tgt[~nothing], beg[~nothing], end[~nothing], win[~nothing]
    end = np.minimum(end, win - 1)
    first = np.concatenate([[0], np.cumsum(windows)])                               # a target's first global window
    total = int(first[-1])
    diff = np.bincount(first[tgt] + beg, minlength=total + 1).astype(np.int64)
    diff -= np.bincount(first[tgt] + end + 1, minlength=total + 1)
    hit = np.cumsum(diff[:total]) > 0
    csum = np.concatenate([[0], np.cumsum(hit)])
    covered = (csum[first[1:]] - csum[first[:-1]]).astype(np.uint32)
    return covered, out_of_range, int(len(tgt))


def keep(covered, windows, percentile, order=None) -> np.ndarray:
    """filter_targets_by_coverage with the visiting order as a parameter -> keep[targets] uint8"""
    n = len(covered)
    visit = range(n) if order is None else [int(t) for t in order]
    cov = []
    total = np.float32(0)
    for t in visit:
        if int(covered[t]) == 0:
            continue
        p = np.float32(np.float32(int(covered[t])) / np.float32(int(windows[t])))
        total = np.float32(total + p)
        cov.append((t, p))
    cov.sort(key=lambda c: c[1])                                                    # (Python's sort is stable)
    out = np.zeros(n, dtype=np.uint8)
    for t, _ in cov:
        out[t] = 1
    limit = np.float32(np.float32(percentile) * total)
    part = np.float32(0)
    for t, p in cov:
        part = np.float32(part + p)
        if part > limit:
            break
        out[t] = 0
    return out


def drop(cands: np.ndarray, keep_mask: np.ndarray) -> np.ndarray:
    """rows with the used entries of kept targets at the front, in their order, zeros behind them"""
    n, stride = cands.shape
    tgt = cands["tgt"].astype(np.int64)
    km = np.concatenate([np.asarray(keep_mask, dtype=np.uint8), [0]])
    stays = used(cands) & (km[np.where(tgt < len(keep_mask), tgt, len(keep_mask))] != 0)
    order = np.argsort(~stays, axis=1, kind="stable")
    out = np.take_along_axis(cands, order, axis=1)
    out[np.arange(stride)[None, :] >= stays.sum(axis=1)[:, None]] = np.zeros((), dtype=cands.dtype)
    return out
