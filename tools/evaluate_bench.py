#!/usr/bin/env python3
"""Measures mc_evaluate_assignments' kernel (taxon_evaluate_kernel) on device-resident (assignment, truth) pairs (a record, not a gate).

No database: a synthetic taxonomy (sequence, species, genus, family, order, class, phylum, domain filled, as tools/classify_bench.py's)
whose table of EVERY taxon -- targets and their ancestors -- has about --taxa rows (default 50 000 and 2 500 000, NCBI's size), and
--reads (5 * 10^6) pairs under three mixes:
    all_right        every read assigned its true target: the walk ends on the first slot
    half_to_phylum   half of the reads as above, half assigned a target of another class of the true one's phylum: a walk of six slots
    ten_taxa         90 % of the truths on ten targets, the rest uniform; the assigned target is a neighbour (same genus, mostly)
Variants: verdicts alone, verdicts + tallies, verdicts + tallies + the coverage counters (a tenth of the taxa are marked uncovered).
Per configuration: HIP events around --inner (10) calls enqueued back to back, the median of --reps (7) such windows after a warm-up,
per call.  The yardsticks, in the same run and measured the same way: a device-to-device copy of the bytes the kernel's arrays hold
(n * 16) and taxon_vote_kernel<true> (mc_classify_candidates with tallies, stride 2, 40 000 targets, uniform reads) on the same n.

Usage:  python tools/evaluate_bench.py [--out profiles/evaluate_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import classify_bench  # noqa: E402  (the synthetic lineages and candidate lists of the vote's measurement)

NUM_RANKS = 21
PER_CLASS, PER_PHYLUM = 6 * 4 * 4 * 3 * 3, 6 * 4 * 4 * 3 * 3 * 3           # targets under one class / one phylum (classify_bench.FANOUT)


def taxon_table(nt: int):
    """the table of every taxon of classify_bench.lineage_table(nt): the targets' rows, then one row per ancestor (its descendants' row
    from its own slot up) -> lin[taxa, 21], rank[taxa], covered[taxa] (a tenth of the species and everything below them: uncovered)"""
    tl = classify_bench.lineage_table(nt)
    taxa = int(tl.max())
    lin = np.zeros((taxa, NUM_RANKS), dtype=np.uint32)
    rank = np.full(taxa, NUM_RANKS, dtype=np.uint8)
    lin[:nt] = tl
    rank[:nt] = 0
    for r in classify_bench.FILLED[1:]:
        ids, first = np.unique(tl[:, r], return_index=True)
        rows = tl[first].copy()
        rows[:, :r] = 0
        lin[ids - 1] = rows
        rank[ids - 1] = r
    covered = np.ones(taxa, dtype=np.uint8)
    species = tl[:, 4]
    off = (species % 10) == 0
    covered[np.flatnonzero(off)] = 0
    covered[np.unique(species[off]) - 1] = 0
    return lin, rank, covered


def pairs(torch, dev, n: int, nt: int, mix: str, seed: int):
    """-> assigned [n, 2] int32 (mc_assignment: taxon, info), truth [n] int32; taxa as index + 1 (targets are the first nt taxa)"""
    g = torch.Generator(device=dev); g.manual_seed(seed)
    t = torch.randint(0, nt, (n,), generator=g, device=dev)
    if mix == "all_right":
        a = t.clone()
    elif mix == "half_to_phylum":
        other = (t // PER_PHYLUM) * PER_PHYLUM + (t % PER_PHYLUM + PER_CLASS + torch.randint(0, PER_CLASS, (n,), generator=g, device=dev)) % PER_PHYLUM
        a = torch.where(torch.rand((n,), generator=g, device=dev) < 0.5, t, torch.clamp(other, max=nt - 1))
    elif mix == "ten_taxa":
        hot = torch.randint(0, nt, (10,), generator=g, device=dev)
        t = torch.where(torch.rand((n,), generator=g, device=dev) < 0.9, hot[torch.randint(0, 10, (n,), generator=g, device=dev)], t)
        a = torch.clamp(t + torch.randint(-12, 13, (n,), generator=g, device=dev), 0, nt - 1)
    else:
        raise ValueError(mix)
    assigned = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    assigned[:, 0] = (a + 1).to(torch.int32)
    return assigned, (t + 1).to(torch.int32).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evaluate_bench.json"))
    ap.add_argument("--reads", type=int, default=5_000_000)
    ap.add_argument("--taxa", type=int, nargs="+", default=[50_000, 2_500_000])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--commit", default=None, help="recorded as it is (where the tree is not a git checkout)")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps: medians of at least 5 windows")
    import torch
    from metacache_amd import api
    if not torch.cuda.is_available():
        sys.exit("evaluate_bench: no GPU (there is nothing to measure without one)")
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
    res = {"date": datetime.datetime.now().isoformat(timespec="seconds"), "commit": commit, "device": torch.cuda.get_device_name(0),
           "reads": n, "table_layout": "rows padded to 128 bytes", "reps": a.reps, "calls_per_window": a.inner, "query_step_ms": 16.4, "runs": []}

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
        # the yardsticks: a copy of the arrays' bytes, and the vote with its tallies on as many reads
        nbytes = n * 16
        src = torch.empty(nbytes, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
        torch.cuda.synchronize()
        copy = window_ms(lambda: db.copy_results(dst.data_ptr(), src.data_ptr(), nbytes, stream=st.cuda_stream))
        db.set_lineages(classify_bench.lineage_table(40_000))
        c = classify_bench.candidate_lists(torch, dev, n, 2, 40_000, "uniform", seed=1)
        out = torch.empty((n, 2), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        vote = window_ms(lambda: db.classify_device(c.data_ptr(), n, 2, out_ptr=out.data_ptr(), stream=st.cuda_stream, tally=True,
                                                    hitmin=5, hitdiff=1.0, lowest=0, highest=19))
        del c, out
        res["copy_ms"], res["copy_ms_min_max"] = copy[0], [copy[1], copy[2]]
        res["vote_tally_ms"], res["vote_tally_ms_min_max"] = vote[0], [vote[1], vote[2]]
        print(json.dumps({"copy_ms": copy[0], "vote_tally_ms": vote[0]}), flush=True)
        verdicts = torch.empty(n, dtype=torch.int32, device=dev)
        for want in a.taxa:
            nt = int(want / 1.2205)                                             # targets, so that targets + ancestors come to about `want`
            lin, rank, covered = taxon_table(nt)
            db.set_taxon_table(lin, rank, covered)
            for mix in ("all_right", "half_to_phylum", "ten_taxa"):
                da, dt = pairs(torch, dev, n, nt, mix, seed=nt % 1000 + len(mix))
                torch.cuda.synchronize()
                for variant, kw in (("verdicts", dict(tally=False)), ("tally", dict(tally=True)), ("tally_coverage", dict(tally=True, coverage=True))):
                    med, lo, hi = window_ms(lambda: db.evaluate_device(da.data_ptr(), dt.data_ptr(), n, verdicts_ptr=verdicts.data_ptr(),
                                                                       stream=st.cuda_stream, **kw))
                    v = verdicts.cpu().numpy().view(api.verdict_dtype)
                    run = {"taxa": len(lin), "table_MB": len(lin) * 128 / 1e6, "mix": mix, "variant": variant, "bytes": nbytes,
                           "kernel_ms": med, "kernel_ms_min_max": [lo, hi], "ratio_to_copy": med / copy[0], "ratio_to_vote": med / vote[0],
                           "GB_per_s": nbytes / med / 1e6, "reads_per_s": n / med * 1e3, "share_of_query_step": med / 16.4,
                           "counted_wrong": float((v["flags"] & 1).mean()), "mean_correct_rank": float(v["correct"].mean())}
                    res["runs"].append(run)
                    print(json.dumps(run), flush=True)
                db.evaluation(reset=True)
                del da, dt
    finally:
        db.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
