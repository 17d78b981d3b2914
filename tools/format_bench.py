#!/usr/bin/env python3
"""Measures mc_format_mappings' three kernels (format_lengths_kernel, tile_scan_kernel, format_write_kernel) on device-resident arrays
(a record, not a gate).

No database: --reads (5 * 10^6) synthetic reads with names of 8 .. 24 bytes, candidate lists of stride 2 and 4 (a quarter of the lists
one entry short, hits 1 .. 300), 40 000 targets whose candidate texts look like accession numbers (11 bytes) and 50 000 result texts of
15 .. 60 bytes, a fifth of the reads unclassified; with -queryids, once with and once without the -tophits column.
Per configuration: HIP events around --inner (5) calls enqueued back to back, the median of --reps (7) such windows after a warm-up,
per call.  The yardstick, in the same run and measured the same way: a device-to-device copy of as many bytes as the call reads from
its arrays (candidates, assignments, names and their offsets) and writes (the lines and their offsets); the table bytes a call reads
depend on the cache and are left out of it, so the ratio is an upper bound of the distance to a copy.

Usage:  python tools/format_bench.py [--out profiles/format_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import datetime
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "format_bench.json"))
    ap.add_argument("--reads", type=int, default=5_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--commit", default=None, help="recorded as it is (where the tree is not a git checkout)")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: medians of at least 5 windows")
    import torch
    from metacache_amd import api
    if not torch.cuda.is_available():
        sys.exit("format_bench: no GPU (there is nothing to measure without one)")
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
        except OSError:
            commit = None
    dev = torch.device("cuda", 0)
    cfg = api.default_config()
    h = C.c_void_p()
    if api.lib().mc_create(C.byref(cfg), C.byref(h)) != 0:
        sys.exit("mc_create: " + api.lib().mc_last_error(None).decode())
    db = api.Database.from_handle(h.value, cfg)
    st = torch.cuda.Stream(device=dev)
    n = a.reads
    rng = np.random.default_rng(1)
    targets, taxa = 40_000, 50_000
    res = {"date": datetime.datetime.now().isoformat(timespec="seconds"), "commit": commit, "device": torch.cuda.get_device_name(0),
           "reads": n, "targets": targets, "result_texts": taxa, "reps": a.reps, "calls_per_window": a.inner, "runs": []}

    def window_ms(call):
        """median over the windows of: events around `inner` calls on the stream, per call"""
        for _ in range(2):
            call()
        st.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(a.inner):
                call()
            e1.record(st)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / a.inner)
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    try:
        lens = rng.integers(15, 61, taxa)
        db.format_set_text(api.TEXT_RESULT, [b"--"] + [b"species:" + b"x" * int(l - 8) for l in lens[1:]])
        db.format_set_text(api.TEXT_CANDIDATE, [b"NC_%06d.1" % t for t in range(targets)])
        name_len = rng.integers(8, 25, n)
        name_off = np.zeros(n + 1, dtype=np.int64)
        name_off[1:] = np.cumsum(name_len)
        names = torch.randint(65, 91, (int(name_off[-1]) + 16,), dtype=torch.uint8, device=dev)
        dname_off = torch.from_numpy(name_off).to(dev)
        g = torch.Generator(device=dev); g.manual_seed(2)
        assigned = torch.zeros((n, 2), dtype=torch.int32, device=dev)
        assigned[:, 0] = torch.where(torch.rand((n,), generator=g, device=dev) < 0.2, 0, torch.randint(1, taxa, (n,), generator=g, device=dev)).to(torch.int32)
        assigned[:, 1] = torch.where(assigned[:, 0] == 0, 21, 4).to(torch.int32)
        line_off = torch.empty(n + 1 + api.FORMAT_SCRATCH, dtype=torch.int64, device=dev)
        opt = api.format_options(b"\t|\t", 112, 127)
        for stride in (2, 4):
            c = torch.zeros((n, stride, 4), dtype=torch.int32, device=dev)
            c[:, :, 0] = torch.randint(0, targets, (n, stride), generator=g, device=dev).to(torch.int32)
            c[:, :, 1] = torch.randint(1, 300, (n, stride), generator=g, device=dev).to(torch.int32)
            c[:, :, 2] = torch.randint(0, 40_000, (n, stride), generator=g, device=dev).to(torch.int32)
            c[:, :, 3] = c[:, :, 2] + 2
            c[: n // 4, stride - 1, 1] = 0
            for tophits in (False, True):
                flags = api.FORMAT_QUERY_IDS | (api.FORMAT_TOPHITS if tophits else 0)
                kw = dict(flags=flags, first_query_id=1, line_off_ptr=line_off.data_ptr(), stream=st.cuda_stream)
                probe = torch.empty(16, dtype=torch.uint8, device=dev)
                db.format_device(opt, c.data_ptr(), stride, assigned.data_ptr(), names.data_ptr(), dname_off.data_ptr(), n, out_ptr=probe.data_ptr(), out_capacity=0, **kw)
                st.synchronize()
                total = int(line_off[n].item())
                out = torch.empty(total + 16, dtype=torch.uint8, device=dev)
                torch.cuda.synchronize()
                med, lo, hi = window_ms(lambda: db.format_device(opt, c.data_ptr(), stride, assigned.data_ptr(), names.data_ptr(), dname_off.data_ptr(), n,
                                                                 out_ptr=out.data_ptr(), out_capacity=total, **kw))
                assert int(line_off[n].item()) == total and int((out[:total] == 10).sum().item()) == n
                nbytes = n * stride * 16 + n * 8 + int(name_off[-1]) + (n + 1) * 8 + total + (n + 1) * 8
                src = torch.empty(nbytes, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
                torch.cuda.synchronize()
                copy = window_ms(lambda: db.copy_results(dst.data_ptr(), src.data_ptr(), nbytes, stream=st.cuda_stream))
                del src, dst
                db.timing(True); db.timing_reset()
                db.format_device(opt, c.data_ptr(), stride, assigned.data_ptr(), names.data_ptr(), dname_off.data_ptr(), n, out_ptr=out.data_ptr(), out_capacity=total, **kw)
                st.synchronize()
                parts = {k: db.timing_get(k)[0] for k in ("format_lengths", "format_write")}
                db.timing(False)
                run = {"stride": stride, "tophits": tophits, "line_bytes": total, "mean_line": total / n, "bytes_moved": nbytes, "call_ms": med,
                       "call_ms_min_max": [lo, hi], "copy_ms": copy[0], "ratio_to_copy": med / copy[0], "GB_per_s": nbytes / med / 1e6,
                       "reads_per_s": n / med * 1e3, "lengths_and_scan_ms": parts["format_lengths"], "write_ms": parts["format_write"]}
                res["runs"].append(run)
                print(json.dumps(run), flush=True)
                del out
            del c
        res["stats"] = db.format_stats()
    finally:
        db.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
