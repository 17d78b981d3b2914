#!/usr/bin/env python3
"""Measures the kernels behind mc_target_hits_* on device-resident candidate lists (a record, not a gate).

The setup of tools/coverage_bench.py: no database, a window table of --targets (40 000) targets, the lineage table of
tools/classify_bench.py, --reads (5 * 10^6) candidate lists of stride 2 and 4, the reads uniform over the targets or 90 % of them on ten.

APPEND, per stride and distribution, all in one run, HIP events around --inner calls enqueued back to back on one stream, the median of
--reps (7) such windows after a warm-up, per call:
    append_ms      target_hits_append_kernel into a log with room for a window's records (the log is emptied before every window)
    mark_ms        coverage_mark_kernel in steady state (a bitmap that holds the batch already) on the same rows
    copy_ms        a device-to-device copy of the rows' n * 16 * stride bytes
COLLECT, per distribution, for --records (10^7 and 10^8) records -- the stride-2 rows appended again and again with other query ids:
    sort_ms, bounds_ms   the block sort + merge passes / the bounds kernel between HIP events on the context's stream (mc_timing_get)
    copy_back_ms         the host's time for the call that copies offsets and records back (the log is sorted by then)
    collect_ms           the host's time for both calls of Database.target_hits_collect: sizes (which sorts), then the arrays
    host_sort_ms         what `mcq` did with the same records before: std::sort of 32-byte Cover records on one thread
                         (tools/host_cover_sort.cpp), on the same box; the median of three runs for 10^7 records, one run beyond
    host_to_device       host_sort_ms / collect_ms

Usage:  python tools/target_hits_bench.py [--out profiles/target_hits_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import datetime
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "target_hits_bench.json"))
    ap.add_argument("--reads", type=int, default=5_000_000)
    ap.add_argument("--targets", type=int, default=40_000)
    ap.add_argument("--strides", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--records", type=int, nargs="+", default=[10_000_000, 100_000_000])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--commit", default=None, help="recorded as it is (where the tree is not a git checkout)")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: medians of at least 5 windows")
    import torch
    from classify_bench import lineage_table
    from coverage_bench import candidate_lists, window_table
    from metacache_amd import api, build
    if not torch.cuda.is_available():
        sys.exit("target_hits_bench: no GPU (there is nothing to measure without one)")
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
        except OSError:
            commit = None
    host = C.CDLL(build.build_cover_sort())
    host.mc_tool_cover_sort_ms.restype = C.c_double
    host.mc_tool_cover_sort_ms.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_int)]
    host.mc_tool_records_in_order.argtypes = [C.c_void_p, C.c_uint64]
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    opt = dict(hitmin=5, lowest=0)
    res = {"date": datetime.datetime.now().isoformat(timespec="seconds"), "commit": commit, "device": torch.cuda.get_device_name(0),
           "reads": a.reads, "targets": a.targets, "options": opt, "reps": a.reps, "calls_per_window": a.inner, "tile": api.target_hits_tile(),
           "append": [], "collect": []}

    def stats(ms):
        return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}

    def window_ms(call, inner, before=None):
        """events around `inner` calls on the stream, per call; `before` runs (and is waited for) ahead of every window"""
        for _ in range(2):
            if before is not None:
                st.synchronize()                                        # (`before` resets on the context's stream: nothing of ours may still run)
                before()
            call()
        st.synchronize()
        ms = []
        for _ in range(a.reps):
            if before is not None:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(inner):
                call()
            e1.record(st)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / inner)
        return stats(ms)

    windows = window_table(a.targets)
    cfg = api.default_config()
    h = C.c_void_p()
    if api.lib().mc_create(C.byref(cfg), C.byref(h)) != 0:
        sys.exit("mc_create: " + api.lib().mc_last_error(None).decode())
    db = api.Database.from_handle(h.value, cfg)
    L = api.lib()

    def empty_log():
        db._check(L.mc_target_hits_collect(db.h, None, 0, None, None, 0, None, None, 1))     # (no arrays, no stats: a reset without a sort)

    try:
        db.load_target_windows(windows)
        db.set_lineages(lineage_table(a.targets))
        for stride in a.strides:
            nbytes = a.reads * 16 * stride
            src = torch.empty(nbytes, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
            torch.cuda.synchronize()
            copy = window_ms(lambda: db.copy_results(dst.data_ptr(), src.data_ptr(), nbytes, stream=st.cuda_stream), a.inner)
            del src, dst
            for dist in ("uniform", "ten_targets"):
                c = candidate_lists(torch, dev, a.reads, stride, windows, dist, seed=a.targets + stride)
                torch.cuda.synchronize()
                db.target_hits_reserve(0)
                db.target_hits_reserve(a.reads * min(stride, 2) * a.inner)                    # (the lists hold two entries at most)
                append = window_ms(lambda: db.target_hits_add_device(c.data_ptr(), a.reads, stride, stream=st.cuda_stream, **opt), a.inner, before=empty_log)
                size = db.target_hits_stats()
                assert size["dropped"] == 0 and size["calls"] == a.inner, size
                db.target_hits_reserve(0)
                db.coverage_counts(reset=True)
                mark = window_ms(lambda: db.coverage_add_device(c.data_ptr(), a.reads, stride, stream=st.cuda_stream, **opt), a.inner)   # (its warm-up calls fill the bitmap)
                run = {"stride": stride, "distribution": dist, "bytes": nbytes, "records_per_call": size["records"] // a.inner,
                       "append_ms": append, "mark_ms": mark, "copy_ms": copy,
                       "append_to_copy": append["median"] / copy["median"], "append_to_mark": append["median"] / mark["median"]}
                res["append"].append(run)
                print(json.dumps(run), flush=True)
                if stride == a.strides[0]:
                    for want in a.records:
                        res["collect"].append(collect_case(a, db, L, host, c, stride, dist, want, opt, st, stats))
                        print(json.dumps(res["collect"][-1]), flush=True)
                del c
        # what a worker of `mcq` pays per batch: the synchronous host-mode call on 4 096 rows of stride 2 (staging copy, kernel, waits)
        rows = np.zeros((4096, 2), dtype=api.cand_dtype)
        rows["tgt"] = np.random.default_rng(1).integers(0, a.targets, size=rows.shape); rows["hits"] = 30; rows["end"] = 2
        db.target_hits_reserve(0)
        wall = []
        for _ in range(200):
            t0 = time.perf_counter()
            db.target_hits_add(rows, hitmin=5)
            wall.append((time.perf_counter() - t0) * 1e3)
        res["host_mode_add_4096_rows_ms"] = stats(wall[20:])
        print(json.dumps(res["host_mode_add_4096_rows_ms"]), flush=True)
        db.target_hits_reserve(0)
    finally:
        db.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


def collect_case(a, db, L, host, c, stride, dist, want, opt, st, stats):
    """`want` records (whole calls of the stride's rows, so a little fewer) in the log, then the two calls of a collect; --reps times"""
    from metacache_amd import api
    db.target_hits_reserve(0)
    db.target_hits_reserve(want)
    db.target_hits_add_device(c.data_ptr(), a.reads, stride, stream=st.cuda_stream, **opt)
    st.synchronize()
    nt, nr = C.c_uint64(), C.c_uint64()
    db._check(L.mc_target_hits_collect(db.h, None, 0, C.byref(nt), None, 0, C.byref(nr), None, 1))
    per_call = int(nr.value)
    calls = max(1, want // per_call)
    records = np.ones(calls * per_call, dtype=api.target_hit_dtype)                          # (written once: the pages exist before anything is timed)
    offsets = np.ones(nt.value + 1, dtype=np.uint64)
    s4 = np.zeros(4, dtype=np.uint64)
    sort, bounds, size_call, back = [], [], [], []
    db.timing(True)
    for rep in range(a.reps + 1):                                                             # (the first is the warm-up)
        db._check(L.mc_target_hits_collect(db.h, None, 0, None, None, 0, None, None, 1))     # empty; then the same rows under other query ids
        for k in range(calls):
            db.target_hits_add_device(c.data_ptr(), a.reads, stride, first_query_id=k * a.reads, stream=st.cuda_stream, **opt)
        st.synchronize()
        db.timing_reset()
        t0 = time.perf_counter()
        db._check(L.mc_target_hits_collect(db.h, None, 0, None, None, 0, C.byref(nr), s4.ctypes.data, 0))                       # sorts
        t1 = time.perf_counter()
        db._check(L.mc_target_hits_collect(db.h, offsets.ctypes.data, nt.value, None, records.ctypes.data, len(records), None, None, 0))
        t2 = time.perf_counter()
        assert nr.value == len(records) and int(s4[1]) == 0, (nr.value, len(records), s4)
        if rep:
            sort.append(db.timing_get("target_hits_sort")[0]); bounds.append(db.timing_get("target_hits_bounds")[0] / 2)        # (two launches: one per call)
            size_call.append((t1 - t0) * 1e3); back.append((t2 - t1) * 1e3)
    db.timing(False)
    assert host.mc_tool_records_in_order(records.ctypes.data, len(records)) == 1, "the device's order"
    # the parent's way with the same records: they reached its vector in the order of the reads, which is no order of the targets -- here
    # the sorted records are dealt out again with a step that is coprime to their number
    step = 1_000_003
    while np.gcd(step, len(records)) != 1:
        step += 2
    hs = []
    for r in range(3 if len(records) <= 20_000_000 else 1):
        unsorted = records[(np.arange(len(records), dtype=np.int64) * step + 7919 * r) % len(records)]
        ok = C.c_int()
        hs.append(host.mc_tool_cover_sort_ms(unsorted.ctypes.data, len(unsorted), C.byref(ok)))
        assert ok.value == 1
        del unsorted
    db.target_hits_reserve(0)
    collect = [x + y for x, y in zip(size_call, back)]
    run = {"distribution": dist, "stride": stride, "records": len(records), "add_calls": calls, "passes": int(np.ceil(np.log2(max(1, -(-len(records) // api.target_hits_tile()))))),
           "sort_ms": stats(sort), "bounds_ms": stats(bounds), "size_call_ms": stats(size_call), "copy_back_ms": stats(back), "collect_ms": stats(collect),
           "host_sort_ms": stats(hs), "host_sort_runs": len(hs)}
    run["host_to_device"] = run["host_sort_ms"]["median"] / run["collect_ms"]["median"]
    run["host_to_device_sort_only"] = run["host_sort_ms"]["median"] / run["sort_ms"]["median"]
    return run


if __name__ == "__main__":
    main()
