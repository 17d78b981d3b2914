"""A plain model of the window sketch (TEST INFRASTRUCTURE): numpy only, no ctypes, nothing shared with oracle/mc_oracle.c.

The operation every device sketcher implements: cut a sequence into windows, take every window's canonical k-mers that hold no
ambiguous character, hash them, keep the `s` smallest DISTINCT hashes in ascending order.

    windows(L, k, w, stride, no_tail)  -> [(first, n), ...]       window rule, stride > w included
    sketch(seq, k, s, w, stride)       -> (feats[nwin, s], counts[nwin])
    facts(seq, k, s, w, stride)        -> Sketch: the same plus per-window facts no implementation decides
                                          (nk, valid, below, dup), with which the device tests prove that their inputs reach the
                                          branches they are there for
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

NONE = 0xFFFFFFFF           # padding of a sketch row; never a feature
_M32 = np.uint64(0xFFFFFFFF)

# A/a = 0, C/c = 1, G/g = 2, T/t/U/u = 3; every other byte is ambiguous (4)
CODE = np.full(256, 4, dtype=np.uint8)
for _letters, _c in (("Aa", 0), ("Cc", 1), ("Gg", 2), ("TtUu", 3)):
    for _ch in _letters:
        CODE[ord(_ch)] = _c


def windows(L: int, k: int, w: int, stride: int, no_tail: bool = False):
    """(first character, characters) of every window that gets a sketch.  A sequence of up to w characters is one window; a longer
    one has a full window at every multiple of the stride that still fits and, unless no_tail, the rest behind the last of them
    (which starts one stride further, possibly beyond the end when stride > w).  Windows of fewer than k characters have no k-mer
    and are not counted."""
    if L <= w:
        return [(0, L)] if L >= k else []
    out = []
    first = 0
    while first + w <= L:
        out.append((first, w))
        first += stride
    if not no_tail and first < L and L - first >= k:
        out.append((first, L - first))
    return out


def tm_hash(x: np.ndarray) -> np.ndarray:
    """Thomas Mueller's 32-bit mix, on uint64 arrays that hold 32-bit values"""
    x = x.astype(np.uint64)
    m = np.uint64(0x45D9F3B)
    s = np.uint64(16)
    x = (((x >> s) ^ x) * m) & _M32
    x = (((x >> s) ^ x) * m) & _M32
    return (x >> s) ^ x


def kmer_hashes(seq: bytes, k: int):
    """-> (hash[nk] uint64, valid[nk] bool) of the k-mers at every position of seq: the hash of the smaller of the k-mer (2 bits per
    base, first base in the highest bits) and its reverse complement; valid = no ambiguous character inside"""
    a = np.frombuffer(bytes(seq), dtype=np.uint8)
    nk = len(a) - k + 1
    if nk <= 0:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=bool)
    code = CODE[a]
    bad = np.concatenate(([0], np.cumsum(code == 4)))
    valid = (bad[k:] - bad[:-k]) == 0
    c = (code & 3).astype(np.uint64)
    fwd = np.zeros(nk, dtype=np.uint64)
    rev = np.zeros(nk, dtype=np.uint64)
    for j in range(k):
        cj = c[j:j + nk]
        fwd |= cj << np.uint64(2 * (k - 1 - j))
        rev |= (np.uint64(3) - cj) << np.uint64(2 * j)
    return tm_hash(np.minimum(fwd, rev)), valid


class Sketch(NamedTuple):
    feats: np.ndarray     # [nwin, s] uint32, ascending distinct, padded with 0xFFFFFFFF
    counts: np.ndarray    # [nwin] uint32
    nk: np.ndarray        # [nwin] k-mers of the window, valid or not
    valid: np.ndarray     # [nwin] k-mers without an ambiguous character
    below: np.ndarray     # [nwin] valid k-mers whose hash lies below the first threshold (first_threshold)
    dup: np.ndarray       # [nwin] the sl smallest valid hashes, counted with multiplicity, contain a repeat
    dup_first: np.ndarray # [nwin] place of the first such repeat among them (the pair dup_first, dup_first + 1), -1: none
    dup_pairs: np.ndarray # [nwin] equal neighbours among them
    below128: np.ndarray  # [nwin] `below` among the window's first 128 k-mers only, and ...
    below256: np.ndarray  # [nwin] ... among its k-mers 128 .. 255 (sketch_window_v3 goes through a window 128 k-mers at a time)
    first: np.ndarray     # [nwin] first character of the window


def first_threshold(s: int, nk: int) -> int:
    """min(floor(7 * sl * 2^32 / (4 * nk)), 0xFFFFFFFF), sl = min(s, nk): the bound below which sketch_window_v3 (kernels.hip: t64 / T)
    collects its candidates in the first pass -- 1.75 times the expected sl-th smallest of nk uniform hashes"""
    sl = min(s, nk)
    return min(((7 * sl) << 32) // (4 * nk), NONE)


def facts(seq: bytes, k: int, s: int, w: int, stride: int, no_tail: bool = False) -> Sketch:
    seq = bytes(seq)
    wins = windows(len(seq), k, w, stride, no_tail)
    n = len(wins)
    feats = np.full((n, s), NONE, dtype=np.uint32)
    counts = np.zeros(n, dtype=np.uint32)
    nks = np.zeros(n, dtype=np.int64)
    nvalid = np.zeros(n, dtype=np.int64)
    below = np.zeros(n, dtype=np.int64)
    dup = np.zeros(n, dtype=bool)
    dup_first = np.full(n, -1, dtype=np.int64)
    dup_pairs = np.zeros(n, dtype=np.int64)
    below128 = np.zeros(n, dtype=np.int64)
    below256 = np.zeros(n, dtype=np.int64)
    h, ok = kmer_hashes(seq, k)
    for i, (first, nch) in enumerate(wins):
        nk = nch - k + 1
        sl = min(s, nk)
        hv = h[first:first + nk][ok[first:first + nk]]
        nks[i] = nk
        nvalid[i] = len(hv)
        T = np.uint64(first_threshold(s, nk))
        below[i] = int((hv < T).sum())
        for lo, dst in ((0, below128), (128, below256)):
            part = slice(first + lo, first + min(lo + 128, nk))
            dst[i] = int((h[part][ok[part]] < T).sum()) if lo < nk else 0
        hv = np.sort(hv[hv != np.uint64(NONE)])
        head = hv[:sl]
        eq = np.flatnonzero(head[1:] == head[:-1])
        dup[i] = eq.size > 0
        dup_pairs[i] = eq.size
        dup_first[i] = eq[0] if eq.size else -1
        keep = np.ones(len(hv), dtype=bool)
        keep[1:] = hv[1:] != hv[:-1]
        d = hv[keep][:sl]
        feats[i, :len(d)] = d
        counts[i] = len(d)
    return Sketch(feats, counts, nks, nvalid, below, dup, dup_first, dup_pairs, below128, below256, np.array([f for f, _ in wins], dtype=np.int64))


def sketch(seq: bytes, k: int, s: int, w: int, stride: int, no_tail: bool = False):
    """-> (feats[nwin, s] uint32 padded with 0xFFFFFFFF, counts[nwin])"""
    r = facts(seq, k, s, w, stride, no_tail)
    return r.feats, r.counts
