#!/usr/bin/env python3
"""Measures the kernels behind mc_coverage_* on device-resident candidate lists (a record, not a gate).

No database: window tables of --targets targets (default 40 000 and 72 000) whose sizes are spread log-normally (sigma 0.5) and add up
to the windows of the 150 Gbp bench collection (1.344 * 10^9 at the default window stride: a bitmap of 168 MB), the lineage table of
tools/classify_bench.py, --reads (5 * 10^6) candidate lists of stride 2 and 4 whose entries cover 1 - 3 windows inside their target,
under two distributions of the reads over the targets:
    uniform      every target and every window equally likely
    ten_targets  90 % of the reads on ten targets, the rest uniform (one sample: the reads pile onto a few genomes)
Per configuration, for the marking kernel WITH the load before the atomic (the shipped form) and WITHOUT it (mc_set_tuning
"coverage_load_first" 0):
    fresh_ms   one call on an empty bitmap (HIP events around the single call, the bitmap cleared before each), median of --reps
    steady_ms  a call on a bitmap that holds the batch already -- the steady state of a real run: events around --inner (10) calls
               enqueued back to back, the median of --reps (7) such windows after a warm-up, per call
and, measured like steady_ms in the same run: coverage_drop_kernel (half of the targets kept, out of place), taxon_vote_kernel<false>
on the same rows, and a device-to-device copy of the rows' n * 16 * stride bytes.  count_kernel_ms is coverage_count_kernel alone
between two HIP events on the context's stream (mc_timing_enable / mc_timing_get), the median of --reps launches on the bitmap that
holds the batch; counts_call_ms is the host's time for the whole mc_coverage_counts call around it (the kernel, two small copies, the wait).

Usage:  python tools/coverage_bench.py [--out profiles/coverage_bench.json]
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
TOTAL_WINDOWS = 1_344_000_000                   # 150.5 Gbp / 112


def window_table(nt: int) -> np.ndarray:
    rng = np.random.default_rng(nt)
    w = rng.lognormal(0.0, 0.5, size=nt)
    return np.maximum(1, np.round(w * (TOTAL_WINDOWS / w.sum()))).astype(np.uint32)


def candidate_lists(torch, dev, n: int, stride: int, windows, dist: str, seed: int):
    nt = len(windows)
    g = torch.Generator(device=dev); g.manual_seed(seed)
    w = torch.from_numpy(windows.astype(np.int64)).to(dev)
    top = torch.randint(0, nt, (n,), generator=g, device=dev)
    if dist == "ten_targets":
        hot = torch.randint(0, nt, (10,), generator=g, device=dev)
        on_hot = torch.rand((n,), generator=g, device=dev) < 0.9
        top = torch.where(on_hot, hot[torch.randint(0, 10, (n,), generator=g, device=dev)], top)
    c = torch.zeros((n, stride, 4), dtype=torch.int32, device=dev)
    hits = torch.randint(20, 61, (n,), generator=g, device=dev)
    for j in range(min(stride, 2)):                                  # as classify_bench: a second candidate of the same genus, the further ones empty
        tgt = top if j == 0 else torch.clamp(top + torch.randint(-12, 13, (n,), generator=g, device=dev), 0, nt - 1)
        length = torch.randint(1, 4, (n,), generator=g, device=dev)
        beg = (torch.rand((n,), generator=g, device=dev, dtype=torch.float64) * w[tgt]).to(torch.int64)
        end = torch.minimum(beg + length - 1, w[tgt] - 1)
        c[:, j, 0] = tgt; c[:, j, 1] = hits if j == 0 else torch.clamp(hits - torch.randint(0, 31, (n,), generator=g, device=dev), min=1)
        c[:, j, 2] = beg; c[:, j, 3] = end
    return c


def reasoning(res) -> str:
    """why `shipped` is shipped, in words, from the figures of the run"""
    runs, sums = res["runs"], res["sum_of_both_cases_ms"]
    med = lambda r, k, w: r[k][w]["median"]
    rng = lambda v: f"{min(v):.2f}-{max(v):.2f}"
    uni = [r for r in runs if r["distribution"] == "uniform"]
    ten = [r for r in runs if r["distribution"] == "ten_targets"]
    return (f"fresh + steady ms summed over the {len(runs)} cases: load_first {sums['load_first']:.2f}, atomic_always {sums['atomic_always']:.2f}; "
            f"the smaller sum is shipped ({res['shipped']}). atomic_always costs the same on a fresh and on a filled bitmap "
            f"(uniform {rng([med(r, 'atomic_always', 'steady_ms') for r in uni])} ms, ten_targets {rng([med(r, 'atomic_always', 'steady_ms') for r in ten])} ms: "
            f"atomics on the same few lines queue); load_first pays the load on a fresh bitmap "
            f"(uniform {rng([med(r, 'load_first', 'fresh_ms') / med(r, 'atomic_always', 'fresh_ms') for r in uni])} x atomic_always) and saves the atomics in steady state "
            f"(uniform {rng([med(r, 'load_first', 'steady_ms') for r in uni])} ms, ten_targets {rng([med(r, 'load_first', 'steady_ms') for r in ten])} ms; "
            f"{rng([r['steady_to_vote'] for r in runs])} x taxon_vote_kernel<false> on the same rows).")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coverage_bench.json"))
    ap.add_argument("--reads", type=int, default=5_000_000)
    ap.add_argument("--targets", type=int, nargs="+", default=[40_000, 72_000])
    ap.add_argument("--strides", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--commit", default=None, help="recorded as it is (where the tree is not a git checkout)")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: medians of at least 5 windows")
    import torch
    from classify_bench import lineage_table
    from metacache_amd import api
    if not torch.cuda.is_available():
        sys.exit("coverage_bench: no GPU (there is nothing to measure without one)")
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
        except OSError:
            commit = None
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    opt = dict(hitmin=5, lowest=0)
    res = {"date": datetime.datetime.now().isoformat(timespec="seconds"), "commit": commit, "device": torch.cuda.get_device_name(0),
           "reads": a.reads, "options": opt, "reps": a.reps, "calls_per_window": a.inner, "total_windows": TOTAL_WINDOWS, "runs": []}

    def stats(ms):
        return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}

    def window_ms(call, inner, before=None):
        """events around `inner` calls on the stream, per call; `before` runs (and is waited for) ahead of every window"""
        if before is None:
            for _ in range(2):
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

    for nt in a.targets:
        windows = window_table(nt)
        cfg = api.default_config()
        h = C.c_void_p()
        if api.lib().mc_create(C.byref(cfg), C.byref(h)) != 0:
            sys.exit("mc_create: " + api.lib().mc_last_error(None).decode())
        db = api.Database.from_handle(h.value, cfg)
        try:
            db.load_target_windows(windows)
            db.set_lineages(lineage_table(nt))
            keep = (np.arange(nt) % 2).astype(np.uint8)
            db.coverage_set_keep(keep)
            for stride in a.strides:
                nbytes = a.reads * 16 * stride
                src = torch.empty(nbytes, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
                votes = torch.empty((a.reads, 2), dtype=torch.int32, device=dev)
                torch.cuda.synchronize()
                copy = window_ms(lambda: db.copy_results(dst.data_ptr(), src.data_ptr(), nbytes, stream=st.cuda_stream), a.inner)
                for dist in ("uniform", "ten_targets"):
                    c = candidate_lists(torch, dev, a.reads, stride, windows, dist, seed=nt + stride)
                    torch.cuda.synchronize()
                    mark = lambda: db.coverage_add_device(c.data_ptr(), a.reads, stride, stream=st.cuda_stream, **opt)
                    run = {"targets": nt, "stride": stride, "distribution": dist, "bytes": nbytes, "bitmap_bytes": int(((windows.astype(np.int64) + 31) // 32).sum() * 4)}
                    for name, flag in (("load_first", 1), ("atomic_always", 0)):
                        db.set_tuning("coverage_load_first", flag)
                        fresh = window_ms(mark, 1, before=lambda: db.coverage_counts(reset=True))
                        db.coverage_counts(reset=True)
                        steady = window_ms(mark, a.inner)               # (its warm-up calls fill the bitmap)
                        run[name] = {"fresh_ms": fresh, "steady_ms": steady}
                    db.set_tuning("coverage_load_first", 1)
                    st.synchronize()
                    nul = C.c_uint64()
                    kern, call = [], []
                    db.timing(True)
                    for _ in range(a.reps + 1):                                  # (one launch per call; the first is the warm-up)
                        db.timing_reset()
                        t0 = time.perf_counter()
                        db._check(api.lib().mc_coverage_counts(db.h, None, None, 0, C.byref(nul), None, 0))
                        call.append((time.perf_counter() - t0) * 1e3)
                        kern.append(db.timing_get("coverage_count_kernel")[0])
                    db.timing(False)
                    run["count_kernel_ms"] = stats(kern[1:]); run["counts_call_ms"] = stats(call[1:])
                    covered, _, cst = db.coverage_counts()
                    run["covered_windows"] = int(covered.sum()); run["covered_targets"] = int((covered > 0).sum())
                    run["drop_ms"] = window_ms(lambda: db.coverage_drop_device(c.data_ptr(), a.reads, stride, dst.data_ptr(), stream=st.cuda_stream), a.inner)
                    run["vote_ms"] = window_ms(lambda: db.classify_device(c.data_ptr(), a.reads, stride, out_ptr=votes.data_ptr(), stream=st.cuda_stream,
                                                                          hitmin=5, hitdiff=1.0, lowest=0, highest=19), a.inner)
                    run["copy_ms"] = copy
                    run["steady_to_vote"] = run["load_first"]["steady_ms"]["median"] / run["vote_ms"]["median"]
                    run["sum_load_first_ms"] = run["load_first"]["fresh_ms"]["median"] + run["load_first"]["steady_ms"]["median"]
                    run["sum_atomic_always_ms"] = run["atomic_always"]["fresh_ms"]["median"] + run["atomic_always"]["steady_ms"]["median"]
                    res["runs"].append(run)
                    print(json.dumps(run), flush=True)
                    del c
                del src, dst, votes
        finally:
            db.close()
    res["sum_of_both_cases_ms"] = {k: float(sum(r["sum_" + k + "_ms"] for r in res["runs"])) for k in ("load_first", "atomic_always")}
    res["shipped"] = min(res["sum_of_both_cases_ms"], key=res["sum_of_both_cases_ms"].get)
    res["reasoning"] = reasoning(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
