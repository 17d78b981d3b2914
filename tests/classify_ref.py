"""Plain numpy model of the ranked-LCA vote (include/metacache_amd.h, "classification"): what mc_classify_candidates must compute.

Written from the rules, one read at a time, with numpy's float32 for the one place that is floating point; the tests compare the
device against it, and it against the reference's own output lines (test_classify_witness_cpu.py)."""
from __future__ import annotations

import numpy as np

NUM_RANKS = 21
UNCLASSIFIED = (0, NUM_RANKS, 0)        # taxon, rank, voters


def lineage_of(lin: np.ndarray, tgt: int) -> np.ndarray:
    """lin[targets, 21]; a target outside the table has a lineage of zeros"""
    return lin[tgt] if 0 <= tgt < len(lin) else np.zeros(NUM_RANKS, dtype=lin.dtype)


def vote(lin: np.ndarray, tgts, hits, hits_min: int, hits_diff, lowest: int, highest: int):
    """one read: tgts / hits of its candidate entries (all `stride` of them) -> (taxon, rank, voters)"""
    n = 0
    while n < len(hits) and int(hits[n]) != 0:      # the list ends at the first entry without hits
        n += 1
    if n == 0:
        return UNCLASSIFIED
    top = lineage_of(lin, int(tgts[0]))
    if lowest == 0:
        r = 0
    else:
        r = next((k for k in range(lowest, NUM_RANKS) if top[k] != 0), NUM_RANKS)
    if r >= NUM_RANKS or top[r] == 0 or int(hits[0]) < hits_min:
        return UNCLASSIFIED
    h0 = int(hits[0])
    threshold = np.float32(h0 - hits_min) * np.float32(hits_diff) if h0 > hits_min else np.float32(0)
    voters = 1
    for i in range(1, n):
        if not (np.float32(int(hits[i])) > threshold):
            break
        voters += 1
        other = lineage_of(lin, int(tgts[i]))
        r = next((k for k in range(r, NUM_RANKS) if top[k] != 0 and top[k] == other[k]), NUM_RANKS)
        if r >= NUM_RANKS or r > highest:
            return UNCLASSIFIED
    if r > highest:
        return UNCLASSIFIED
    return int(top[r]), r, min(voters, 255)


def vote_all(lin: np.ndarray, cands: np.ndarray, hits_min: int, hits_diff, lowest: int, highest: int) -> np.ndarray:
    """cands[n, stride] with fields tgt, hits -> int64 [n, 3]: taxon, rank, voters"""
    out = np.zeros((len(cands), 3), dtype=np.int64)
    T, H = cands["tgt"], cands["hits"]
    for i in range(len(cands)):
        out[i] = vote(lin, T[i], H[i], hits_min, hits_diff, lowest, highest)
    return out


def vote_all_fast(lin: np.ndarray, cands: np.ndarray, hits_min: int, hits_diff, lowest: int, highest: int) -> np.ndarray:
    """vote_all for millions of rows: the same rules, every step taken for all reads at once (checked against vote() by the tests)"""
    n, stride = cands.shape
    linx = np.vstack([lin.astype(np.int64), np.zeros((1, NUM_RANKS), dtype=np.int64)])       # last row: the lineage of zeros
    nt = len(lin)
    T = np.where(cands["tgt"] < nt, cands["tgt"], nt).astype(np.int64)
    H = cands["hits"].astype(np.int64)
    top = linx[T[:, 0]]                                                                       # [n, 21]
    ranks = np.arange(NUM_RANKS)

    def first_rank(mask, start):
        """per row the first k >= start[row] with mask[row, k], NUM_RANKS if none"""
        m = mask & (ranks[None, :] >= start[:, None])
        return np.where(m.any(axis=1), m.argmax(axis=1), NUM_RANKS)

    if lowest == 0:
        r = np.where(top[:, 0] != 0, 0, NUM_RANKS)
    else:
        r = first_rank(top != 0, np.full(n, lowest))
    alive = (H[:, 0] != 0) & (r < NUM_RANKS) & (H[:, 0] >= hits_min)                           # still classified
    d = np.where(H[:, 0] > hits_min, H[:, 0] - hits_min, 0).astype(np.uint32)
    threshold = np.where(H[:, 0] > hits_min, d.astype(np.float32) * np.float32(hits_diff), np.float32(0)).astype(np.float32)
    voting = alive.copy()                                                                      # the walk over the candidates goes on
    voters = alive.astype(np.int64)
    for j in range(1, stride):
        voting &= (H[:, j] != 0) & (H[:, j].astype(np.float32) > threshold)
        if not voting.any():
            break
        other = linx[T[:, j]]
        r2 = first_rank((top != 0) & (top == other), np.minimum(r, NUM_RANKS))
        failed = voting & ((r2 >= NUM_RANKS) | (r2 > highest))
        r = np.where(voting, r2, r)
        voters += voting
        alive &= ~failed
        voting &= ~failed
    alive &= r <= highest
    out = np.zeros((n, 3), dtype=np.int64)
    rr = np.where(alive, r, 0)
    out[:, 0] = np.where(alive, top[np.arange(n), rr], 0)
    out[:, 1] = np.where(alive, r, NUM_RANKS)
    out[:, 2] = np.where(alive, np.minimum(voters, 255), 0)
    return out
