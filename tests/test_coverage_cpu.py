"""CPU: the mc_coverage_* calls without a device -- the names, the order of the checks (arguments first, then state), and
mc_coverage_keep (pure host) against the model of coverage_ref.py; the model's marking against a loop over single windows."""
import ctypes as C
import os

import numpy as np
import pytest

import coverage_ref
from metacache_amd import api

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MC_OK, MC_ERR_INVALID, MC_ERR_STATE = 0, -1, -6
NAMES = ("mc_coverage_add", "mc_coverage_counts", "mc_coverage_keep", "mc_coverage_set_keep", "mc_coverage_drop")


def test_the_five_names_are_exported_and_declared():
    L = C.CDLL(api._build.build_library())
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "metacache_amd.h")).read()
    for n in NAMES:
        assert hasattr(L, n) and n in api.EXPORTS and ("int " + n + "(") in header
    assert "#define MC_COVERAGE_HOST 1" in header and api.COVERAGE_HOST == 1


def test_error_order_arguments_first_then_state():
    L = api.lib()
    h = C.c_void_p()
    assert L.mc_open_metadata(os.path.join(GOLDEN, "toy32").encode(), C.byref(h)) == MC_OK      # lineages, but no device
    try:
        cands = np.zeros((8, 2), dtype=api.cand_dtype)
        out = np.zeros((8, 2), dtype=api.cand_dtype)

        def add(ctx=h, c=cands.ctypes.data, n=4, stride=2, hitmin=0, lowest=0, flags=api.COVERAGE_HOST):
            return L.mc_coverage_add(ctx, c, n, stride, hitmin, lowest, flags, None)

        def drop(ctx=h, c=cands.ctypes.data, n=4, stride=2, flags=api.COVERAGE_HOST, o=out.ctypes.data):
            return L.mc_coverage_drop(ctx, c, n, stride, flags, o, None)

        assert add(ctx=None) == MC_ERR_INVALID
        assert add(c=None) == MC_ERR_INVALID
        assert add(stride=0) == MC_ERR_INVALID and add(stride=0, n=0) == MC_ERR_INVALID          # looked at even when there is nothing to do
        assert add(lowest=-1) == MC_ERR_INVALID and add(lowest=21) == MC_ERR_INVALID and add(lowest=21, n=0) == MC_ERR_INVALID
        assert add(flags=2) == MC_ERR_INVALID and add(flags=3) == MC_ERR_INVALID and add(flags=1 << 24) == MC_ERR_INVALID
        assert L.mc_last_error(h)
        assert add(n=0) == MC_OK and add(n=0, c=None) == MC_OK and add(n=0, flags=0) == MC_OK
        assert add() == MC_ERR_STATE and add(flags=0) == MC_ERR_STATE and add(lowest=20) == MC_ERR_STATE
        assert add(stride=0) == MC_ERR_INVALID                                                   # bad arguments win over the missing state

        assert drop(ctx=None) == MC_ERR_INVALID
        assert drop(c=None) == MC_ERR_INVALID and drop(o=None) == MC_ERR_INVALID
        assert drop(stride=0) == MC_ERR_INVALID and drop(flags=2) == MC_ERR_INVALID
        assert drop(o=cands.ctypes.data + 16) == MC_ERR_INVALID                                  # shifted by one entry
        assert drop(o=cands.ctypes.data + 4 * 2 * 16 - 16) == MC_ERR_INVALID                     # the last entry of in is the first of out
        assert drop(c=cands.ctypes.data + 16, o=cands.ctypes.data) == MC_ERR_INVALID
        assert drop(o=cands.ctypes.data + 4 * 2 * 16) == MC_ERR_STATE                            # right behind it: no overlap
        assert drop(o=cands.ctypes.data) == MC_ERR_STATE                                         # in place is allowed: what is missing is the state
        assert drop() == MC_ERR_STATE and drop(n=0, c=None, o=None) == MC_ERR_STATE

        st = np.zeros(4, dtype=np.uint64)
        assert L.mc_coverage_counts(None, None, None, 0, None, st.ctypes.data, 0) == MC_ERR_INVALID
        assert L.mc_coverage_counts(h, None, None, 0, None, st.ctypes.data, 0) == MC_ERR_STATE
        keep = np.ones(4, dtype=np.uint8)
        assert L.mc_coverage_set_keep(None, keep.ctypes.data, 4) == MC_ERR_INVALID
        assert L.mc_coverage_set_keep(h, keep.ctypes.data, 4) == MC_ERR_STATE
        assert L.mc_coverage_set_keep(h, None, 0) == MC_ERR_STATE
    finally:
        L.mc_destroy(h)


def raw_keep(covered, windows, percentile, order=None, num_targets=None):
    covered = np.ascontiguousarray(covered, dtype=np.uint32); windows = np.ascontiguousarray(windows, dtype=np.uint32)
    n = len(covered) if num_targets is None else num_targets
    keep = np.full(max(n, 1), 7, dtype=np.uint8)
    o = None if order is None else np.ascontiguousarray(order, dtype=np.uint32)
    rc = api.lib().mc_coverage_keep(covered.ctypes.data, windows.ctypes.data, n, None if o is None else o.ctypes.data, 0 if o is None else len(o),
                                    percentile, keep.ctypes.data)
    return rc, keep[:n]


def test_keep_refuses_bad_arguments():
    cov, win = [1, 2, 3], [4, 4, 4]
    for p in (-0.01, 1.01, float("nan"), float("inf"), -float("inf")):
        assert raw_keep(cov, win, p)[0] == MC_ERR_INVALID
    assert raw_keep(cov, win, 0.5, order=[0, 1, 1])[0] == MC_ERR_INVALID          # repeated
    assert raw_keep(cov, win, 0.5, order=[0, 3])[0] == MC_ERR_INVALID             # beyond the targets
    assert raw_keep(cov, win, 0.5, order=[2, 0, 1])[0] == MC_OK
    L = api.lib()
    k = np.zeros(3, dtype=np.uint8)
    c = np.array(cov, dtype=np.uint32)
    assert L.mc_coverage_keep(None, c.ctypes.data, 3, None, 0, 0.5, k.ctypes.data) == MC_ERR_INVALID
    assert L.mc_coverage_keep(c.ctypes.data, None, 3, None, 0, 0.5, k.ctypes.data) == MC_ERR_INVALID
    assert L.mc_coverage_keep(c.ctypes.data, c.ctypes.data, 3, None, 0, 0.5, None) == MC_ERR_INVALID
    assert L.mc_coverage_keep(None, None, 0, None, 0, 0.5, None) == MC_OK          # no targets: nothing to do
    with pytest.raises(api.McError):
        api.coverage_keep(cov, win, -1.0)


@pytest.mark.parametrize("percentile", [0.0, 1.0, 0.5, 0.1, 0.25, 0.9, 0.999, 1e-6])
def test_keep_equals_the_model(percentile):
    rng = np.random.default_rng(5)
    n = 400
    windows = rng.integers(1, 3000, size=n).astype(np.uint32)
    covered = np.minimum(rng.integers(0, 3000, size=n), windows).astype(np.uint32)
    covered[rng.random(n) < 0.3] = 0                                                # never hit: skipped, not kept
    for order in (None, rng.permutation(n), rng.permutation(n)[: n // 2]):
        rc, got = raw_keep(covered, windows, percentile, order)
        want = coverage_ref.keep(covered, windows, percentile, order)
        assert rc == MC_OK and np.array_equal(got, want), (percentile, order is None)
        visited = np.ones(n, bool) if order is None else np.isin(np.arange(n), order)
        assert not got[(covered == 0) | ~visited].any()
        if percentile == 0.0:
            assert np.array_equal(got != 0, (covered > 0) & visited)                # nothing is dropped
        if percentile == 1.0:
            assert got.sum() <= 1                                                   # at most the rounding of the last sum keeps one
    assert np.array_equal(api.coverage_keep(covered, windows, percentile), coverage_ref.keep(covered, windows, percentile))


def test_percent_rule_of_the_wrapper():
    for v in (0.0, 0.3, 1.0):
        assert api.percentile_factor(v) == float(np.float32(v))
    for v in (30, 1.5, 99, 100):
        assert api.percentile_factor(v) == float(np.float32(np.float64(np.float32(v)) * 0.01))
    cov, win = [1, 2, 3, 4], [4, 4, 4, 4]
    assert np.array_equal(api.coverage_keep(cov, win, 30), api.coverage_keep(cov, win, api.percentile_factor(30)))


def test_equal_coverages_fall_in_visiting_order():
    """a stable sort: of equal coverages the ones visited first are dropped first"""
    covered = np.array([5, 5, 5, 5, 5, 5, 9, 0], dtype=np.uint32)
    windows = np.array([10, 10, 10, 10, 10, 10, 10, 10], dtype=np.uint32)
    # sum = 3.9; 0.3 * 3.9 = 1.17: two of the six halves go (0.5, 1.0), the third (1.5) stops it
    rc, got = raw_keep(covered, windows, 0.3)
    assert rc == MC_OK and got.tolist() == [0, 0, 1, 1, 1, 1, 1, 0]
    rc, got = raw_keep(covered, windows, 0.3, order=[5, 4, 3, 2, 1, 0, 6, 7])
    assert rc == MC_OK and got.tolist() == [1, 1, 1, 1, 0, 0, 1, 0]
    rc, got = raw_keep(covered, windows, 0.3, order=[6, 3, 0, 5])                   # sum 2.4, limit 0.72: 3 goes, 0 stops it; 1, 2, 4 not visited
    assert rc == MC_OK and got.tolist() == [1, 0, 0, 0, 0, 1, 1, 0]
    for order in (None, [5, 4, 3, 2, 1, 0, 6, 7], [6, 3, 0, 5]):
        assert np.array_equal(raw_keep(covered, windows, 0.3, order)[1], coverage_ref.keep(covered, windows, 0.3, order))


def test_the_float_sum_follows_the_visiting_order():
    """Two orders whose float sums differ, and with them the targets that go.  N targets with 1 of 2^25 windows covered (covP = 2^-25)
    and one fully covered target (covP = 1): visited FIRST, the 1 absorbs every 2^-25 that follows (half an ulp of 1 is 2^-24) and the
    sum is 1; visited LAST it is added to N * 2^-25 = 2^-10, sum 1 + 2^-10.  With percentile 2^-11 the limits are 2^-11 and
    2^-11 + 2^-21 = (2^14 + 16) * 2^-25: the small targets go in their visiting order while k * 2^-25 <= limit (every number here
    is exact in float) -- 2^14 of them in the first order, 2^14 + 16 in the second."""
    N = 1 << 15
    covered = np.ones(N + 1, dtype=np.uint32); windows = np.full(N + 1, 1 << 25, dtype=np.uint32)
    covered[N] = windows[N] = 1000
    p = float(np.float32(2.0 ** -11))
    big_first = np.concatenate([[N], np.arange(N)])
    rc, a = raw_keep(covered, windows, p, big_first)
    assert rc == MC_OK
    rc, b = raw_keep(covered, windows, p, None)                                     # ascending ids: the big one last
    assert rc == MC_OK
    assert not a[: 1 << 14].any() and a[1 << 14:].all()
    assert not b[: (1 << 14) + 16].any() and b[(1 << 14) + 16:].all()
    assert np.array_equal(a, coverage_ref.keep(covered, windows, p, big_first)) and np.array_equal(b, coverage_ref.keep(covered, windows, p, None))


def mark_window_by_window(windows, lin, cands, hits_min, lowest):
    """the rules of the header, one entry and one window at a time"""
    hit = [set() for _ in windows]
    outside = marked = 0
    for row in cands:
        for c in row:
            tgt, hits, beg, end = (int(c[f]) for f in ("tgt", "hits", "beg", "end"))
            if hits == 0:
                break
            lineage = lin[tgt] if tgt < len(lin) else np.zeros(21, dtype=np.uint32)
            t = int(lineage[0]) if lowest == 0 else next((int(x) for x in lineage[lowest:] if x), 0)
            if hits < hits_min or t == 0:
                continue
            if tgt >= len(windows) or beg > end or beg >= int(windows[tgt]):
                outside += 1
                continue
            if end >= int(windows[tgt]):
                outside += 1
                end = int(windows[tgt]) - 1
            marked += 1
            hit[tgt].update(range(beg, end + 1))
    return np.array([len(s) for s in hit], dtype=np.uint32), outside, marked


@pytest.mark.parametrize("stride,lowest", [(1, 0), (3, 0), (4, 5), (7, 20)])
def test_the_models_marking_equals_a_loop_over_windows(stride, lowest):
    rng = np.random.default_rng(stride)
    nt = 60
    windows = rng.choice([1, 2, 31, 32, 33, 64, 65, 200], size=nt).astype(np.uint32)
    lin = rng.integers(0, 50, size=(nt + 5, 21)).astype(np.uint32)                  # (more lineages than window counts)
    lin[rng.random(lin.shape) < 0.6] = 0
    c = np.zeros((1500, stride), dtype=api.cand_dtype)
    c["tgt"] = rng.integers(0, nt + 8, size=c.shape)
    c["hits"] = rng.integers(0, 9, size=c.shape)
    c["beg"] = rng.integers(0, 210, size=c.shape)
    c["end"] = c["beg"] + rng.integers(-2, 40, size=c.shape).clip(-1)
    for hm in (0, 4):
        got = coverage_ref.mark(windows, lin, c, hm, lowest)
        want = mark_window_by_window(windows, lin, c, hm, lowest)
        assert np.array_equal(got[0], want[0]) and got[1:] == want[1:], (stride, lowest, hm)
        assert got[1] > 0 and got[2] > 0


def test_the_models_drop():
    c = np.zeros((3, 4), dtype=api.cand_dtype)
    c["tgt"] = [[0, 1, 2, 3], [1, 9, 1, 0], [2, 2, 0, 1]]
    c["hits"] = [[9, 8, 7, 6], [5, 4, 3, 2], [5, 0, 4, 4]]
    c["beg"] = 1; c["end"] = 2
    got = coverage_ref.drop(c, np.array([0, 1, 1], dtype=np.uint8))                 # targets 0, 3 and 9 go
    assert got["tgt"].tolist() == [[1, 2, 0, 0], [1, 1, 0, 0], [2, 0, 0, 0]]
    assert got["hits"].tolist() == [[8, 7, 0, 0], [5, 3, 0, 0], [5, 0, 0, 0]]
    assert got["end"].tolist() == [[2, 2, 0, 0], [2, 2, 0, 0], [2, 0, 0, 0]]
