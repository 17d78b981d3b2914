#!/usr/bin/env python3
"""Measures mc_classify_candidates' kernel (taxon_vote_kernel) on device-resident candidate lists (a record, not a gate).

No database: a synthetic lineage table (sequence, species, genus, family, order, class, phylum, domain filled, as taxonomies of real
collections are) for --targets targets (default 40 000 and 72 000), --reads (5 * 10^6) candidate lists of stride 2 and 4, with and
without the tallies, under two distributions of the reads over the targets:
    uniform      every target equally likely
    ten_taxa     90 % of the reads on ten targets, the rest uniform (one sample: the reads pile onto a few taxa)
A list's top candidate has 20 - 60 hits; the second one is a target of the same genus with up to 30 hits fewer (it votes when it is
above the threshold: -hitmin 5, -hitdiff 1.0 as the command line's defaults), the further ones are empty.
Per configuration: HIP events around --inner (10) calls enqueued back to back, the median of --reps (7) such windows after a warm-up,
per call.  The yardstick, in the same run and measured the same way: a device-to-device copy of the bytes the kernel's arrays hold,
n * (16 * stride + 8).  `ratio_to_copy` = kernel time / copy time; `query_step_ms` (16.4: the query step of 5 * 10^6 reads the vote
would follow) stands beside it for scale.

Usage:  python tools/classify_bench.py [--out profiles/classify_bench.json]
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
NUM_RANKS = 21
FILLED = (0, 4, 6, 10, 12, 14, 16, 19)          # sequence, species, genus, family, order, class, phylum, domain
FANOUT = (6, 4, 4, 3, 3, 3, 1000000)            # targets per species, species per genus, ... everything under one domain


def lineage_table(nt: int) -> np.ndarray:
    """[nt, 21] taxon index + 1; targets that are neighbours by number share the lower ancestors"""
    lin = np.zeros((nt, NUM_RANKS), dtype=np.uint32)
    lin[:, 0] = np.arange(1, nt + 1)
    nxt, group = nt + 1, np.arange(nt, dtype=np.int64)
    for r, f in zip(FILLED[1:], FANOUT):
        group = group // f
        lin[:, r] = nxt + group
        nxt += int(group.max()) + 1
    return lin


def candidate_lists(torch, dev, n: int, stride: int, nt: int, dist: str, seed: int):
    g = torch.Generator(device=dev); g.manual_seed(seed)
    top = torch.randint(0, nt, (n,), generator=g, device=dev)
    if dist == "ten_taxa":
        hot = torch.randint(0, nt, (10,), generator=g, device=dev)
        on_hot = torch.rand((n,), generator=g, device=dev) < 0.9
        top = torch.where(on_hot, hot[torch.randint(0, 10, (n,), generator=g, device=dev)], top)
    c = torch.zeros((n, stride, 4), dtype=torch.int32, device=dev)
    hits = torch.randint(20, 61, (n,), generator=g, device=dev)
    c[:, 0, 0] = top; c[:, 0, 1] = hits; c[:, 0, 2] = 10; c[:, 0, 3] = 12
    if stride > 1:
        c[:, 1, 0] = torch.clamp(top + torch.randint(-12, 13, (n,), generator=g, device=dev), 0, nt - 1)      # (24 targets to a genus)
        c[:, 1, 1] = torch.clamp(hits - torch.randint(0, 31, (n,), generator=g, device=dev), min=1)
        c[:, 1, 2] = 10; c[:, 1, 3] = 12
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "classify_bench.json"))
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
    from metacache_amd import api
    if not torch.cuda.is_available():
        sys.exit("classify_bench: no GPU (there is nothing to measure without one)")
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
    opt = dict(hitmin=5, hitdiff=1.0, lowest=0, highest=19)
    res = {"date": datetime.datetime.now().isoformat(timespec="seconds"), "commit": commit, "device": torch.cuda.get_device_name(0),
           "reads": a.reads, "options": opt, "reps": a.reps, "calls_per_window": a.inner, "query_step_ms": 16.4, "runs": []}

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
        for nt in a.targets:
            db.set_lineages(lineage_table(nt))
            for stride in a.strides:
                nbytes = a.reads * (16 * stride + 8)
                out = torch.empty((a.reads, 2), dtype=torch.int32, device=dev)
                src = torch.empty(nbytes, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
                torch.cuda.synchronize()
                copy = window_ms(lambda: db.copy_results(dst.data_ptr(), src.data_ptr(), nbytes, stream=st.cuda_stream))
                for dist in ("uniform", "ten_taxa"):
                    c = candidate_lists(torch, dev, a.reads, stride, nt, dist, seed=nt + stride)
                    torch.cuda.synchronize()
                    for tally in (False, True):
                        med, lo, hi = window_ms(lambda: db.classify_device(c.data_ptr(), a.reads, stride, out_ptr=out.data_ptr(), stream=st.cuda_stream,
                                                                           tally=tally, **opt))
                        got = out.cpu().numpy().view(api.assignment_dtype).reshape(a.reads)
                        run = {"targets": nt, "stride": stride, "distribution": dist, "tally": tally, "bytes": nbytes,
                               "kernel_ms": med, "kernel_ms_min_max": [lo, hi], "copy_ms": copy[0], "copy_ms_min_max": [copy[1], copy[2]],
                               "ratio_to_copy": med / copy[0], "GB_per_s": nbytes / med / 1e6, "reads_per_s": a.reads / med * 1e3,
                               "share_of_query_step": med / 16.4, "unclassified": float((got["taxon"] == 0).mean()),
                               "more_than_one_voter": float((got["voters"] > 1).mean()), "distinct_taxa": int(np.unique(got["taxon"]).size)}
                        res["runs"].append(run)
                        print(json.dumps(run), flush=True)
                    del c
                db.tally(reset=True)
    finally:
        db.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
