#!/usr/bin/env python3
"""Measures mc_parse_mates (parse.hip, DESIGN.md 7h "mates") on seeded synthetic mate files: --pairs (10^7) pairs of 150 bp, FASTQ beside
FASTQ and FASTA beside FASTA (the records of tools/parse_bench.py; the two files differ in their seed).

 (a) mc_parse_mates on bytes that are resident on the device against mc_parse_records(MC_PARSE_PAIRS) on the interleaved file of the
     same reads -- the code path that existed before, the baseline -- between HIP events, the two alternating in one process: the
     median, minimum and maximum of --reps (7) calls after a warm-up.  n1 + n2 is at most 2^31: the files go in pieces of whole pairs.
 (b) one slot of --slot-pairs (65 536) pairs: mc_batch_add_file_mates against a numpy cut of the same records and mc_batch_add pair by
     pair inside the clock (mc_batch_add_bulk takes single reads only, so the host side pays one call through the interpreter per
     pair: this is what a Python caller had, not what a C caller had); each with submit, wait and clear; alternating, --reps rounds.
 (c) `mcq query -pairfiles -no-map` on the FASTA files' first --cli-pairs (10^6) pairs with MCQ_PARSE_DEVICE unset and set to 2,
     alternating, --cli-reps (3) runs each: the job time and the workers' summed parse+add of MCQ_PROFILE.

Usage:  python tools/parse_mates_bench.py --db tests/golden/toy32 [--out profiles/parse_mates.json]
"""
from __future__ import annotations

import argparse
import datetime
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from parse_bench import spread, synthetic  # noqa: E402


def bench_kernels(db, api, torch, a1, a2, reps):
    dev = torch.device("cuda", 0)
    n, reclen = a1.shape
    per_piece = min(n, ((1 << 31) - 32) // (2 * reclen))
    ms = {"mates": [0.0] * reps, "pairs_interleaved": [0.0] * reps}
    stream = torch.cuda.Stream(device=dev)
    pieces = 0
    for p0 in range(0, n, per_piece):
        m = min(per_piece, n - p0)
        nb = m * reclen
        d1, d2 = torch.from_numpy(a1[p0:p0 + m].reshape(-1)).to(dev), torch.from_numpy(a2[p0:p0 + m].reshape(-1)).to(dev)
        both = torch.from_numpy(np.stack([a1[p0:p0 + m], a2[p0:p0 + m]], axis=1).reshape(-1)).to(dev)      # the records alternate
        seq_cap, names_cap, mr = 2 * m * 152 + 16, m * 11, 2 * m
        d = dict(hdr=torch.empty(2 * mr, dtype=torch.int32, device=dev), qinfo=torch.empty(4 * m, dtype=torch.int32, device=dev),
                 seq=torch.empty(seq_cap, dtype=torch.uint8, device=dev), names=torch.empty(names_cap, dtype=torch.uint8, device=dev),
                 name_off=torch.empty(m + 1, dtype=torch.int64, device=dev), max_win=torch.empty(m, dtype=torch.int32, device=dev),
                 status=torch.zeros(10, dtype=torch.int64, device=dev))
        out = dict(hdr_ptr=d["hdr"].data_ptr(), qinfo_ptr=d["qinfo"].data_ptr(), seq_ptr=d["seq"].data_ptr(), seq_capacity=seq_cap, names_ptr=d["names"].data_ptr(),
                   names_capacity=names_cap, name_off_ptr=d["name_off"].data_ptr(), max_win_ptr=d["max_win"].data_ptr(), status_ptr=d["status"].data_ptr(), max_records=mr)
        wsb = max(api.parse_mates_scratch_bytes(nb, nb, mr), api.parse_scratch_bytes(2 * nb))
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        calls = {"mates": lambda: db.parse_mates_device(d1.data_ptr(), nb, d2.data_ptr(), nb, workspace_ptr=ws.data_ptr(), workspace_bytes=wsb, stream=stream.cuda_stream, **out),
                 "pairs_interleaved": lambda: db.parse_device(both.data_ptr(), 2 * nb, workspace_ptr=ws.data_ptr(), workspace_bytes=wsb, pairs=True, stream=stream.cuda_stream, **out)}
        seqs = {}
        for k, call in calls.items():                                            # warm-up, and the two must agree
            call()
            torch.cuda.synchronize()
            st = d["status"].cpu().numpy()
            assert int(st[4]) == 0 and int(st[0]) == 2 * m and int(st[1]) == m, (k, st)
            seqs[k] = (d["seq"][:int(st[2])].clone(), d["qinfo"].clone())
        assert torch.equal(seqs["mates"][0], seqs["pairs_interleaved"][0]) and torch.equal(seqs["mates"][1], seqs["pairs_interleaved"][1])
        for r in range(reps):
            for k, call in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(stream):
                    e0.record(); call(); e1.record()
                torch.cuda.synchronize()
                ms[k][r] += e0.elapsed_time(e1)
        pieces += 1
        del d1, d2, both, d, ws, seqs
    return {"pairs": n, "bytes_of_both_files": int(a1.size + a2.size), "pieces": pieces, "mc_parse_mates_ms": spread(ms["mates"]),
            "mc_parse_records_pairs_interleaved_ms": spread(ms["pairs_interleaved"])}


def bench_slot(db, api, a1, a2, head, slot_pairs, reps):
    import ctypes as C
    L = api.lib()
    b1, b2 = a1[:slot_pairs], a2[:slot_pairs]
    r1, r2 = b1.reshape(-1), b2.reshape(-1)
    res = api.McResults()

    def finish():
        db._check(L.mc_batch_submit(db.h, 0, 0))
        db._check(L.mc_batch_wait(db.h, 0, C.byref(res)))
        n = res.num_queries
        db._check(L.mc_batch_clear(db.h, 0))
        return n

    def bulk():
        t = time.perf_counter()
        s1 = np.ascontiguousarray(b1[:, head:head + 150]).reshape(-1)                          # the cut
        s2 = np.ascontiguousarray(b2[:, head:head + 150]).reshape(-1)
        m1, m2, mw = s1.tobytes(), s2.tobytes(), 2 + 300 // db.stride
        for i in range(slot_pairs):                                                             # (mc_batch_add_bulk takes single reads: pairs go one by one)
            assert L.mc_batch_add(db.h, 0, m1[i * 150:i * 150 + 150], 150, m2[i * 150:i * 150 + 150], 150, mw) == 0
        assert finish() == slot_pairs
        return (time.perf_counter() - t) * 1e3

    def file_mates():
        t = time.perf_counter()
        assert L.mc_batch_add_file_mates(db.h, 0, r1.ctypes.data, r1.size, r2.ctypes.data, r2.size, 0) == 0
        assert finish() == slot_pairs
        return (time.perf_counter() - t) * 1e3

    bulk(); file_mates()
    a, b = [], []
    for _ in range(reps):
        a.append(bulk()); b.append(file_mates())
    return {"slot_pairs": slot_pairs, "slot_bytes": int(r1.size + r2.size), "host_cut_and_mc_batch_add_ms": spread(a), "mc_batch_add_file_mates_ms": spread(b)}


def bench_cli(build, db_path, a1, a2, cli_pairs, reps):
    rows = {"off": [], "2": []}
    with tempfile.TemporaryDirectory() as tmp:
        p1, p2 = os.path.join(tmp, "r1.fa"), os.path.join(tmp, "r2.fa")
        a1[:cli_pairs].tofile(p1)
        a2[:cli_pairs].tofile(p2)
        for _ in range(reps):
            for sw in ("off", "2"):
                env = {k: v for k, v in os.environ.items() if k != "MCQ_PARSE_DEVICE"}
                env["MCQ_PROFILE"] = "1"
                if sw != "off":
                    env["MCQ_PARSE_DEVICE"] = sw
                r = subprocess.run([build.MCQ, "query", db_path, p1, p2, "-pairfiles", "-no-map", "-out", os.path.join(tmp, "out.txt")], capture_output=True, text=True, env=env, timeout=1200)
                assert r.returncode == 0, r.stderr[-2000:]
                m = re.search(r"total ([\d.e+-]+) ms; summed over (\d+) workers: parse\+add ([\d.e+-]+) ms", r.stderr)
                p = re.search(r"reads parsed on the device: (\d+) batches, (\d+) bytes, (\d+) records, (\d+) batches parsed on the host", r.stderr)
                rows[sw].append({"job_ms": float(m.group(1)), "workers": int(m.group(2)), "parse_add_ms_summed": float(m.group(3)),
                                 "device_batches": int(p.group(1)) if p else 0, "host_batches": int(p.group(4)) if p else None})
    return {sw: {"job_ms": spread([x["job_ms"] for x in v]), "parse_add_ms_summed": spread([x["parse_add_ms_summed"] for x in v]), "runs": v} for sw, v in rows.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--db", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parse_mates.json"))
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--slot-pairs", type=int, default=65536)
    ap.add_argument("--cli-pairs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cli-reps", type=int, default=3)
    ap.add_argument("--only-cli", action="store_true", help="(c) alone")
    ap.add_argument("--commit", default="unknown", help="recorded as it is")
    a = ap.parse_args()
    import torch
    from metacache_amd import api, build
    res = {"date": datetime.datetime.now(datetime.timezone.utc).isoformat(timespec="seconds"), "commit": a.commit, "device": torch.cuda.get_device_name(0),
           "tile": api.parse_tile(), "reps": a.reps}
    db = api.Database.open(a.db, max_candidates=2, slot_max_queries=a.slot_pairs, slot_max_chars=a.slot_pairs * 2 * 330 + 64)
    try:
        for kind in (("fasta",) if a.only_cli else ("fastq", "fasta")):
            a1, head = synthetic(a.pairs, kind == "fastq", seed=1)
            a2, _ = synthetic(a.pairs, kind == "fastq", seed=2)
            print(f"{kind}: {a.pairs} pairs made", file=sys.stderr, flush=True)
            res[kind] = {}
            if not a.only_cli:
                res[kind]["kernels"] = bench_kernels(db, api, torch, a1, a2, a.reps)
                print(f"{kind}: kernels measured", file=sys.stderr, flush=True)
                res[kind]["slot"] = bench_slot(db, api, a1, a2, head, min(a.slot_pairs, a.pairs), a.reps)
            if kind == "fasta" and a.cli_pairs:
                res[kind]["cli"] = bench_cli(build, a.db, a1, a2, min(a.cli_pairs, a.pairs), a.cli_reps)
            print(json.dumps({kind: {k: v for k, v in res[kind].items()}})[:3000], flush=True)
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
            del a1, a2
    finally:
        db.close()


if __name__ == "__main__":
    main()
