"""CPU: the argument checks of mc_merge_results_* that need no device, on an mc_open_metadata context: every MC_ERR_INVALID comes before
any device call, then MC_ERR_STATE names what the context lacks."""
import ctypes as C
import os

import numpy as np

import merge_results_cases as cases
from metacache_amd import api

INVALID, UNSUPPORTED, STATE = -1, -5, -6


def test_argument_checks_need_no_device():
    L = api.lib()
    h = C.c_void_p()
    assert L.mc_open_metadata(os.path.join(cases.GOLDEN, "toy32").encode(), C.byref(h)) == api.MC_OK
    try:
        data = np.frombuffer(cases.line(1, b"r0", [(9, 5)]) + b"\0" * 64, dtype=np.uint8).copy()
        n = len(cases.line(1, b"r0", [(9, 5)]))
        buf = np.zeros(1024, dtype=np.uint64)                      # (its address is only compared, never read: no device)
        base = buf.ctypes.data + (-buf.ctypes.data) % 16
        status = np.zeros(8, dtype=np.uint64)
        need = api.merge_results_scratch_bytes(n)
        assert need >= 64 and api.merge_results_tile() >= 256

        def add(ctx=h, bytes_ptr=data.ctypes.data, nbytes=n, col=2, flags=api.MERGE_HOST, status_ptr=status.ctypes.data, ws=None, ws_bytes=0):
            return L.mc_merge_results_add(ctx, bytes_ptr, nbytes, col, 0, flags, status_ptr, ws, ws_bytes, None)

        assert add(ctx=None) == INVALID
        assert add(bytes_ptr=None) == INVALID and add(nbytes=0) == INVALID and add(nbytes=(1 << 31) + 1) == INVALID
        assert add(col=0) == INVALID and add(flags=4) == INVALID and add(flags=api.MERGE_HOST | 8) == INVALID
        assert add(status_ptr=None) == INVALID
        dev = dict(flags=0, bytes_ptr=base + 1024, status_ptr=base + 2048, ws=base + 4096, ws_bytes=need)
        assert add(**{**dev, "ws": None}) == INVALID and add(**{**dev, "ws_bytes": need - 1}) == INVALID
        assert add(**{**dev, "bytes_ptr": base + 1025}) == INVALID and add(**{**dev, "ws": base + 4100}) == INVALID
        assert add(**{**dev, "status_ptr": base + 2052}) == INVALID
        assert add(**dev) == STATE and add() == STATE and b"no device" in L.mc_last_error(h)
        assert not status.any()

        ids = np.arange(1, 4, dtype=np.int64)
        assert L.mc_merge_results_set_taxids(None, ids.ctypes.data, 3) == INVALID
        assert L.mc_merge_results_set_taxids(h, None, 3) == INVALID
        assert L.mc_merge_results_set_taxids(h, ids.ctypes.data, 3) == INVALID      # one id per row of the context's taxon table
        nt = C.c_uint64()
        pl = C.c_void_p()
        assert L.mc_db_taxon_table(h, C.byref(pl), None, None, C.byref(nt)) == api.MC_OK and nt.value > 3
        dup = np.arange(1, nt.value + 1, dtype=np.int64)
        dup[-1] = dup[0]
        assert L.mc_merge_results_set_taxids(h, dup.ctypes.data, nt.value) == INVALID and b"two rows" in L.mc_last_error(h)
        dup[-1] = nt.value
        assert L.mc_merge_results_set_taxids(h, dup.ctypes.data, nt.value) == STATE   # regular ids: the context has no device

        assert L.mc_merge_results_begin(None, 10, 2, 4) == INVALID
        assert L.mc_merge_results_begin(h, 10, 0, 4) == INVALID and L.mc_merge_results_begin(h, 1 << 32, 2, 4) == INVALID
        assert L.mc_merge_results_begin(h, 10, 33, 4) == UNSUPPORTED
        assert L.mc_merge_results_begin(h, 10, 16, 4) == STATE
        assert L.mc_merge_results_reserve(None, 10) == INVALID and L.mc_merge_results_reserve(h, 1 << 32) == INVALID
        assert L.mc_merge_results_reserve(h, 10) == STATE

        out = np.zeros(16, dtype=np.uint64)
        assert L.mc_merge_results_lists(None, 0, 1, api.MERGE_HOST, out.ctypes.data, None, None, None) == INVALID
        assert L.mc_merge_results_lists(h, 0, 1, 2, out.ctypes.data, None, None, None) == INVALID
        assert L.mc_merge_results_lists(h, 0, 1, api.MERGE_HOST, None, None, None, None) == INVALID
        assert L.mc_merge_results_lists(h, 0, 1, 0, base + 4, None, None, None) == INVALID
        assert L.mc_merge_results_lists(h, 0, 1, 0, base, base + 2, None, None) == INVALID
        assert L.mc_merge_results_lists(h, 0, 1, api.MERGE_HOST, out.ctypes.data, None, None, None) == STATE

        def classify(ctx=h, opt=None, flags=1, count=1, out_ptr=out.ctypes.data, **kw):
            o = api.classify_options(**kw) if opt is None else opt
            return L.mc_merge_results_classify(ctx, C.byref(o) if o is not False else None, flags, 0, count, out_ptr, None)

        assert classify(ctx=None) == INVALID and classify(opt=False) == INVALID and classify(flags=4) == INVALID
        assert classify(lowest=21) == INVALID and classify(highest=-1) == INVALID and classify(lowest=6, highest=4) == INVALID
        assert classify(hitdiff=-1.0) == INVALID and classify(hitdiff=float("nan")) == INVALID
        assert classify(out_ptr=None) == INVALID and classify(flags=0, out_ptr=base + 4) == INVALID
        assert classify() == STATE

        st = np.ones(6, dtype=np.uint64)
        assert L.mc_merge_results_stats(h, st.ctypes.data) == 0 and not st.any() and L.mc_merge_results_stats(h, None) == INVALID
        L.mc_merge_results_end(h)
        L.mc_merge_results_end(None)
    finally:
        L.mc_destroy(h)
