#!/usr/bin/env python3
"""Measures the all-hits column on device-resident arrays: mc_format_matches (matches_kernel<false>, tile_scan_kernel,
matches_kernel<true>) and mc_format_mappings_with, which copies the column into the lines (a record, not a gate).

No database: synthetic location lists of 100, 1 000 and 5 000 locations per read (--locations in all, 2 * 10^7, so 200 000, 20 000 and
4 000 reads) in runs of 1 .. 3 equal entries, 40 000 targets whose texts look like accession numbers (11 bytes), the window form
(text/window:count,).  The lines: -queryids, names of 8 .. 24 bytes, candidate lists of stride 2 with -tophits, result texts of
15 .. 60 bytes, a fifth of the reads unclassified.
Per configuration and call: HIP events around --inner (5) calls enqueued back to back, the median of --reps (7) such windows after a
warm-up, per call.  The yardstick, in the same run and measured the same way: a device-to-device copy of as many bytes as the call
reads from its arrays and writes (mc_format_matches: the locations and their offsets, the pieces and theirs; mc_format_mappings_with:
candidates, assignments, names, pieces and the three offset arrays, the lines and their offsets); the table bytes a call reads depend
on the cache and are left out of it, so the ratio is an upper bound of the distance to a copy.

Usage:  python tools/matches_bench.py [--out profiles/matches_bench.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matches_bench.json"))
    ap.add_argument("--locations", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--commit", default=None, help="recorded as it is (where the tree is not a git checkout)")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: medians of at least 5 windows")
    import torch
    from metacache_amd import api
    if not torch.cuda.is_available():
        sys.exit("matches_bench: no GPU (there is nothing to measure without one)")
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
    rng = np.random.default_rng(1)
    targets, taxa, stride = 40_000, 50_000, 2
    res = {"date": datetime.datetime.now().isoformat(timespec="seconds"), "commit": commit, "device": torch.cuda.get_device_name(0),
           "locations": a.locations, "targets": targets, "result_texts": taxa, "reps": a.reps, "calls_per_window": a.inner, "runs": []}

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

    def copy_ms(nbytes):
        src = torch.empty(nbytes, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
        torch.cuda.synchronize()
        return window_ms(lambda: db.copy_results(dst.data_ptr(), src.data_ptr(), nbytes, stream=st.cuda_stream))[0]

    try:
        lens = rng.integers(15, 61, taxa)
        db.format_set_text(api.TEXT_RESULT, [b"--"] + [b"species:" + b"x" * int(l - 8) for l in lens[1:]])
        accessions = [b"NC_%06d.1" % t for t in range(targets)]
        db.format_set_text(api.TEXT_CANDIDATE, accessions)
        db.format_matches_set_text(accessions)
        opt = api.format_options(b"\t|\t", 112, 127)
        g = torch.Generator(device=dev); g.manual_seed(2)
        for per_read in (100, 1000, 5000):
            n = a.locations // per_read
            total = n * per_read
            # runs of 1 .. 3 entries; run r is (target, window) = (r // 50 mod targets, r mod 50): neighbours differ, targets ascend
            run_len = rng.integers(1, 4, total // 2 + 2 * n + 4096)
            r = np.arange(len(run_len), dtype=np.uint64)
            keys = (((r // np.uint64(50)) % np.uint64(targets)) << np.uint64(32)) | (r % np.uint64(50))
            hits = np.repeat(keys, run_len)[:total]
            assert len(hits) == total
            dhits = torch.from_numpy(hits.view(np.int64)).to(dev)
            dhit_off = torch.arange(0, total + 1, per_read, dtype=torch.int64, device=dev)
            piece_off = torch.empty(n + 1 + api.FORMAT_SCRATCH, dtype=torch.int64, device=dev)
            probe = torch.empty(16, dtype=torch.uint8, device=dev)
            mkw = dict(flags=api.MATCHES_WINDOWS, piece_off_ptr=piece_off.data_ptr(), stream=st.cuda_stream)
            db.format_matches_device(dhits.data_ptr(), dhit_off.data_ptr(), n, out_ptr=probe.data_ptr(), out_capacity=0, **mkw)
            st.synchronize()
            piece_bytes = int(piece_off[n].item())
            pieces = torch.empty(piece_bytes + 16, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            column = lambda: db.format_matches_device(dhits.data_ptr(), dhit_off.data_ptr(), n, out_ptr=pieces.data_ptr(), out_capacity=piece_bytes, **mkw)
            m_med, m_lo, m_hi = window_ms(column)
            runs_in_pieces = int((pieces[:piece_bytes] == 44).sum().item())           # (every run ends in its comma)
            assert int(piece_off[n].item()) == piece_bytes and runs_in_pieces >= total // 3
            m_bytes = total * 8 + (n + 1) * 8 + piece_bytes + (n + 1) * 8
            m_copy = copy_ms(m_bytes)
            # the lines around the column
            name_len = rng.integers(8, 25, n)
            name_off = np.zeros(n + 1, dtype=np.int64)
            name_off[1:] = np.cumsum(name_len)
            names = torch.randint(65, 91, (int(name_off[-1]) + 16,), dtype=torch.uint8, device=dev)
            dname_off = torch.from_numpy(name_off).to(dev)
            assigned = torch.zeros((n, 2), dtype=torch.int32, device=dev)
            assigned[:, 0] = torch.where(torch.rand((n,), generator=g, device=dev) < 0.2, 0, torch.randint(1, taxa, (n,), generator=g, device=dev)).to(torch.int32)
            assigned[:, 1] = torch.where(assigned[:, 0] == 0, 21, 4).to(torch.int32)
            c = torch.zeros((n, stride, 4), dtype=torch.int32, device=dev)
            c[:, :, 0] = torch.randint(0, targets, (n, stride), generator=g, device=dev).to(torch.int32)
            c[:, :, 1] = torch.randint(1, 300, (n, stride), generator=g, device=dev).to(torch.int32)
            line_off = torch.empty(n + 1 + api.FORMAT_SCRATCH, dtype=torch.int64, device=dev)
            lkw = dict(flags=api.FORMAT_QUERY_IDS | api.FORMAT_TOPHITS, first_query_id=1, line_off_ptr=line_off.data_ptr(), stream=st.cuda_stream,
                       extra_ptr=pieces.data_ptr(), extra_off_ptr=piece_off.data_ptr())
            db.format_device(opt, c.data_ptr(), stride, assigned.data_ptr(), names.data_ptr(), dname_off.data_ptr(), n, out_ptr=probe.data_ptr(), out_capacity=0, **lkw)
            st.synchronize()
            line_bytes = int(line_off[n].item())
            out = torch.empty(line_bytes + 16, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            lines = lambda: db.format_device(opt, c.data_ptr(), stride, assigned.data_ptr(), names.data_ptr(), dname_off.data_ptr(), n,
                                             out_ptr=out.data_ptr(), out_capacity=line_bytes, **lkw)
            l_med, l_lo, l_hi = window_ms(lines)
            assert int(line_off[n].item()) == line_bytes and int((out[:line_bytes] == 10).sum().item()) == n
            assert int((out[:line_bytes] == 44).sum().item()) >= runs_in_pieces
            l_bytes = n * stride * 16 + n * 8 + int(name_off[-1]) + 3 * (n + 1) * 8 + piece_bytes + line_bytes
            l_copy = copy_ms(l_bytes)
            db.timing(True); db.timing_reset()
            column(); lines()
            st.synchronize()
            parts = {k: db.timing_get(k)[0] for k in ("matches_lengths", "matches_write", "format_lengths", "format_write")}
            db.timing(False)
            run = {"locations_per_read": per_read, "reads": n, "runs": runs_in_pieces, "piece_bytes": piece_bytes, "line_bytes": line_bytes,
                   "matches": {"call_ms": m_med, "call_ms_min_max": [m_lo, m_hi], "bytes_moved": m_bytes, "copy_ms": m_copy, "ratio_to_copy": m_med / m_copy,
                               "locations_per_s": total / m_med * 1e3, "lengths_and_scan_ms": parts["matches_lengths"], "write_ms": parts["matches_write"]},
                   "mappings_with": {"call_ms": l_med, "call_ms_min_max": [l_lo, l_hi], "bytes_moved": l_bytes, "copy_ms": l_copy, "ratio_to_copy": l_med / l_copy,
                                     "GB_per_s": l_bytes / l_med / 1e6, "lengths_and_scan_ms": parts["format_lengths"], "write_ms": parts["format_write"]}}
            res["runs"].append(run)
            print(json.dumps(run), flush=True)
            del dhits, dhit_off, pieces, out, c, names
        res["matches_stats"] = db.format_matches_stats()
        res["format_stats"] = db.format_stats()
    finally:
        db.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
