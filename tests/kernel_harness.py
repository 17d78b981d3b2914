"""ctypes side of tests/cpp/kernel_harness.hip (libmckharness.so): the sorted path's device stages driven with chosen inputs
(TEST INFRASTRUCTURE, next to cpuref.py and scale_util.py).

    scan(values, stride, ...)                    launch_scan_u32
    order_sort(n, lists, ...)                    launch_gw_order + launch_gw_segsort
    sorted_cands(n, lists, layout, ...)          gw_sorted_cands_kernel through launch_big_cands

Every call hands host arrays over; the library validates them before it touches the device and answers with one of the codes
below (HarnessError.code), so these calls can be made -- and must fail -- where there is no device.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "metacache_amd", "csrc")

(OK, ERR_HIP, ERR_ARG, ERR_COUNT, ERR_LENGTH, ERR_RANGE, ERR_OVERLAP, ERR_PADDING, ERR_WINDOW, ERR_ORDER, ERR_MAXWIN, ERR_K,
 ERR_QUERY, ERR_TABLE) = range(14)
NAMES = ["OK", "HIP", "ARG", "COUNT", "LENGTH", "RANGE", "OVERLAP", "PADDING", "WINDOW", "ORDER", "MAXWIN", "K", "QUERY", "TABLE"]

UNTOUCHED32 = 0xA5A5A5A5          # qflag / hitScan / scan outputs the kernels did not write
cand_fields = ("tgt", "hits", "beg", "end")


class HarnessError(RuntimeError):
    def __init__(self, code: int, what: str):
        super().__init__(f"{what}: KH_ERR_{NAMES[code] if 0 <= code < len(NAMES) else code}")
        self.code = code


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        from metacache_amd import api, build
        api.lib()                                   # the product library first (it brings the HIP runtime the process already has)
        # (MC_KHARNESS_LIB: another build of the harness, beside the MC_AMD_LIB it was linked against -- see api.lib())
        L = C.CDLL(os.environ.get("MC_KHARNESS_LIB") or build.build_kernel_harness())
        vp, u32, u64, i = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
        L.kh_constants.argtypes = [vp]
        L.kh_constants.restype = None
        L.kh_scan_tmp_bytes.argtypes = [u32]
        L.kh_scan_tmp_bytes.restype = u64
        L.kh_order_temp_bytes.argtypes = [u32, u32]
        L.kh_order_temp_bytes.restype = u64
        L.kh_segsort_temp_bytes.argtypes = [u32, u32, u64]
        L.kh_segsort_temp_bytes.restype = u64
        L.kh_gw_layout.argtypes = [u32, vp, u32, vp, vp, vp, u64]
        L.kh_gw_layout.restype = u64
        L.kh_scan.argtypes = [vp, u32, u32, i, i, i, vp, vp, vp]
        L.kh_order_sort.argtypes = [u32, u32, vp, vp, vp, u64, i, vp, vp, vp]
        L.kh_sorted_cands.argtypes = [u32, u32, vp, vp, vp, u64, vp, vp, vp, u32, vp, u32, u32, vp, vp, vp, vp, vp]
        _lib = L
    return _lib


def constants() -> dict:
    c = np.zeros(8, np.uint32)
    lib().kh_constants(_p(c))
    keys = ["kGwMaxKept", "kGwGap", "kFlagDone", "kFlagCands", "kCntSorted", "kCntSortedBig", "kCounterWords", "kSideSorted"]
    return dict(zip(keys, map(int, c)))


def source_constant(file: str, name: str) -> int:
    """a `constexpr uint32_t NAME = <integer product>` of a kernel file's own (unnamed) namespace, read from the source"""
    txt = open(os.path.join(CSRC, file)).read()
    m = re.search(r"\b" + name + r"\s*=\s*([^,;]+)[,;]", txt)
    assert m, (file, name)
    expr = m.group(1).strip()
    if re.fullmatch(r"[0-9u* ]+", expr):
        return int(eval(expr.replace("u", "")))                                   # noqa: S307 (digits, '*' and blanks only)
    factors = [source_constant(file, f.strip()) for f in expr.split("*")]        # a product of other constants of the file
    return int(np.prod(factors))


# ---- the compact store's numbering ------------------------------------------------------------------------------------------
class GwLayout:
    """gw = gwBase[target] + window,  gwBase[0] = gap,  gwBase[t + 1] = gwBase[t] + windows(t) + gap  (DeviceTable, csrc/kernels.h);
    base / shift / dir come from the harness library, i.e. are the arrays kh_sorted_cands gives the kernel."""

    def __init__(self, windows, gap: int = 1024):
        self.windows = _u32(windows)
        self.gap = int(gap)
        nt = len(self.windows)
        self.base = np.zeros(nt + 1, np.uint32)
        shift = C.c_uint32()
        nd = lib().kh_gw_layout(nt, _p(self.windows), self.gap, _p(self.base), C.byref(shift), None, 0)
        if nd == 0:
            raise HarnessError(ERR_TABLE, "kh_gw_layout")
        self.dir = np.zeros(nd, np.uint32)
        lib().kh_gw_layout(nt, _p(self.windows), self.gap, None, None, _p(self.dir), nd)
        self.shift = int(shift.value)

    def numbers(self, tgt, win) -> np.ndarray:
        """(target, window) arrays -> global window numbers (uint32)"""
        tgt = np.asarray(tgt, dtype=np.int64)
        win = np.asarray(win, dtype=np.int64)
        assert np.all(win < self.windows[tgt].astype(np.int64))
        return (self.base[tgt].astype(np.int64) + win).astype(np.uint32)

    def split(self, gw):
        """global window numbers -> (target, window); the numbers must be some target's windows"""
        gw = np.asarray(gw, dtype=np.int64)
        tgt = np.searchsorted(self.base.astype(np.int64), gw, side="right") - 1
        win = gw - self.base[tgt].astype(np.int64)
        assert np.all(tgt >= 0) and np.all(tgt < len(self.windows)) and np.all(win < self.windows[tgt].astype(np.int64))
        return tgt.astype(np.uint32), win.astype(np.uint32)

    def locations(self, gw) -> np.ndarray:
        """global window numbers -> the oracle's (target << 32 | window) list"""
        t, w = self.split(gw)
        return (t.astype(np.uint64) << np.uint64(32)) | w.astype(np.uint64)


# ---- the calls --------------------------------------------------------------------------------------------------------------
def scan(values, stride: int = 1, n: int | None = None, want32: bool = True, want64: bool = True, want_host: bool = True):
    """-> (out32[n + 1] | None, out64[n + 1] | None, host total | None) of the exclusive scan of values[i * stride]"""
    values = _u32(values)
    if n is None:
        n = len(values) // stride if stride else 0
    o32 = np.zeros(n + 1, np.uint32) if want32 else None
    o64 = np.zeros(n + 1, np.uint64) if want64 else None
    tot = np.zeros(1, np.uint64) if want_host else None
    rc = lib().kh_scan(_p(values), stride, n, int(want32), int(want64), int(want_host), _p(o32), _p(o64), _p(tot))
    if rc:
        raise HarnessError(rc, "kh_scan")
    return o32, o64, (int(tot[0]) if want_host else None)


def pack_lists(lists, sentinel: int | None = None, gaps=None, rng=None):
    """lists of numbers -> (lengths, offsets, pool): the lists one behind the other, `gaps[i]` sentinel words in front of list i (and one
    run behind the last list) when a sentinel is given"""
    lengths = np.array([len(x) for x in lists], dtype=np.uint32)
    if sentinel is None:
        gap = np.zeros(len(lists) + 1, np.int64)
    elif gaps is None:
        gap = (rng or np.random.default_rng(1)).integers(0, 5, len(lists) + 1)
        gap[-1] = 3
    else:
        gap = np.asarray(gaps, dtype=np.int64)
    offsets = (np.cumsum(np.concatenate(([0], lengths[:-1].astype(np.int64)))) + np.cumsum(gap[:-1])).astype(np.int64)
    total = int(lengths.sum() + gap.sum())
    pool = np.full(max(total, 1), 0 if sentinel is None else sentinel, dtype=np.uint32)
    for off, x in zip(offsets, lists):
        pool[off:off + len(x)] = x
    return lengths, offsets.astype(np.uint32), pool


def order_sort(n: int, lengths, offsets, pool, second_stream: bool = False):
    """-> (side list after ordering [nlists], the sort's output pool, the input pool after the run)"""
    lengths, offsets, pool = _u32(lengths), _u32(offsets), _u32(pool)
    side = np.zeros(max(len(lengths), 1), np.uint32)
    out = np.zeros(len(pool), np.uint32)
    after = np.zeros(len(pool), np.uint32)
    rc = lib().kh_order_sort(n, len(lengths), _p(lengths), _p(offsets), _p(pool), len(pool), int(second_stream), _p(side), _p(out), _p(after))
    if rc:
        raise HarnessError(rc, "kh_order_sort")
    return side[:len(lengths)], out, after


def sorted_cands(n: int, lengths, offsets, pool, max_win, q, qhits, layout: GwLayout, K: int, taxkey=None):
    """-> (cands[n, K] structured {tgt, hits, beg, end}, qflag[n], hitScan[n], midCount[kCntSortedBig])"""
    lengths, offsets, pool = _u32(lengths), _u32(offsets), _u32(pool)
    max_win, q, qhits = _u32(max_win), _u32(q), _u32(qhits)
    tk = None if taxkey is None else _u32(taxkey)
    assert tk is None or len(tk) == len(layout.windows)
    assert len(max_win) == len(q) == len(qhits) == len(lengths) == len(offsets)
    cands = np.zeros((max(n, 1), max(K, 1), 4), np.uint32)
    qflag = np.zeros(max(n, 1), np.uint32)
    hitscan = np.zeros(max(n, 1), np.uint32)
    big = np.zeros(1, np.uint32)
    rc = lib().kh_sorted_cands(n, len(lengths), _p(lengths), _p(offsets), _p(pool), len(pool), _p(max_win), _p(q), _p(qhits),
                               len(layout.windows), _p(layout.windows), layout.gap, K, _p(tk), _p(cands), _p(qflag), _p(hitscan), _p(big))
    if rc:
        raise HarnessError(rc, "kh_sorted_cands")
    rec = np.zeros((n, K), dtype=[(f, "<u4") for f in cand_fields])
    for j, f in enumerate(cand_fields):
        rec[f] = cands[:n, :K, j]
    return rec, qflag[:n], hitscan[:n], int(big[0])
