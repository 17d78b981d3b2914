#!/usr/bin/env python3
"""Measures the device parse (parse.hip) on seeded synthetic files: --reads (10^7) reads of 150 bp, FASTA and FASTQ, every
record of one length (a header line of 13 bytes, one sequence line, '\\n' line ends).

 (a) mc_parse_records alone, on bytes that are resident on the device, between HIP events: the median, minimum and maximum of --reps (7)
     calls after a warm-up.  The bytes it reads once plus the bytes it writes, over that time, are set against the 6.29 TB/s a float4
     copy reaches on the MI355X -- the call reads the input FIVE times (one pass per layer, parse.hip), so its own traffic is larger
     than the numerator.  A range takes at most 2^31 bytes: the FASTQ file goes in pieces of whole records.
 (b) one slot of --slot-reads (65 536) reads: mc_batch_add_bulk with the cutting and packing on the host inside the clock -- here numpy
     slicing of records that all have one length, which is the cheapest cut there is, not what a line-by-line reader costs -- against
     mc_batch_add_file_bytes; each with submit, wait and clear; the two alternate in one process, --reps rounds.
 (c) `mcq query -no-map` and `-tophits -queryids` on the FASTA file's first --cli-reads (10^6) reads, with and without
     MCQ_PARSE_DEVICE=1, alternating, --cli-reps (3) runs each: wall time and the `parse+add` share of MCQ_PROFILE.  The run without
     the switch takes the code path of the commit before this one.

Usage:  python tools/parse_bench.py --db tests/golden/toy32 [--out-dir profiles]
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
HBM_COPY_TBS = 6.29                                   # measured float4 copy on the MI355X


def synthetic(n, fastq, seed=1):
    """-> (file bytes as uint8 [n, record length], header bytes per record incl. marker and '\\n')"""
    rng = np.random.default_rng(seed)
    L = 150
    head = np.frombuffer((">" if not fastq else "@").encode() + b"r0000000000\n", dtype=np.uint8)
    reclen = len(head) + L + 1 + ((2 + L + 1) if fastq else 0)
    a = np.empty((n, reclen), dtype=np.uint8)
    a[:, :len(head)] = head
    ids = np.arange(n, dtype=np.int64)
    for k in range(10):
        a[:, 2 + k] = 48 + (ids // 10 ** (9 - k)) % 10
    a[:, len(head):len(head) + L] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n, L), dtype=np.uint8)]
    a[:, len(head) + L] = 10
    if fastq:
        a[:, len(head) + L + 1] = ord("+")
        a[:, len(head) + L + 2] = 10
        a[:, len(head) + L + 3:len(head) + 2 * L + 3] = ord("I")
        a[:, -1] = 10
    return a, len(head)


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def bench_kernels(db, api, torch, arr, reps):
    dev = torch.device("cuda", 0)
    n, reclen = arr.shape
    per_piece = min(n, ((1 << 31) - 16) // reclen)
    total_ms, pieces, moved = [0.0] * reps, 0, 0
    stream = torch.cuda.Stream(device=dev)
    for p0 in range(0, n, per_piece):
        m = min(per_piece, n - p0)
        nbytes = m * reclen
        d_in = torch.from_numpy(arr[p0:p0 + m].reshape(-1)).to(dev)
        seq_cap, names_cap = m * 152 + 16, m * 11
        d = dict(hdr=torch.empty(2 * m, dtype=torch.int32, device=dev), qinfo=torch.empty(4 * m, dtype=torch.int32, device=dev),
                 seq=torch.empty(seq_cap, dtype=torch.uint8, device=dev), names=torch.empty(names_cap, dtype=torch.uint8, device=dev),
                 name_off=torch.empty(m + 1, dtype=torch.int64, device=dev), max_win=torch.empty(m, dtype=torch.int32, device=dev),
                 status=torch.zeros(8, dtype=torch.int64, device=dev))
        wsb = api.parse_scratch_bytes(nbytes)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)

        def call():
            db.parse_device(d_in.data_ptr(), nbytes, hdr_ptr=d["hdr"].data_ptr(), qinfo_ptr=d["qinfo"].data_ptr(), seq_ptr=d["seq"].data_ptr(), seq_capacity=seq_cap,
                            names_ptr=d["names"].data_ptr(), names_capacity=names_cap, name_off_ptr=d["name_off"].data_ptr(), max_win_ptr=d["max_win"].data_ptr(),
                            status_ptr=d["status"].data_ptr(), max_records=m, workspace_ptr=ws.data_ptr(), workspace_bytes=wsb,
                            stream=stream.cuda_stream)

        call()
        torch.cuda.synchronize()
        st = d["status"].cpu().numpy()
        assert int(st[4]) == 0 and int(st[0]) == m, st
        moved += nbytes + int(st[2]) + int(st[3]) + m * (8 + 16 + 8 + 4)
        for r in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record(); call(); e1.record()
            torch.cuda.synchronize()
            total_ms[r] += e0.elapsed_time(e1)
        pieces += 1
        del d_in, d, ws
    s = spread(total_ms)
    return {"reads": n, "file_bytes": int(arr.size), "pieces": pieces, "bytes_read_once_plus_written": moved, "ms": s,
            "tb_per_s_median": moved / (s["median"] * 1e-3) / 1e12, "share_of_hbm_copy_rate": moved / (s["median"] * 1e-3) / 1e12 / HBM_COPY_TBS}


def bench_slot(db, api, arr, head, slot_reads, reps):
    import ctypes as C
    L = api.lib()
    block = arr[:slot_reads]
    raw = block.reshape(-1)
    res = api.McResults()

    def finish():
        db._check(L.mc_batch_submit(db.h, 0, 0))
        db._check(L.mc_batch_wait(db.h, 0, C.byref(res)))
        n = res.num_queries
        db._check(L.mc_batch_clear(db.h, 0))
        return n

    def bulk():
        t = time.perf_counter()
        seqs = np.ascontiguousarray(block[:, head:head + 150]).reshape(-1)                    # the cut
        offs = np.arange(slot_reads + 1, dtype=np.uint64) * 150
        added = L.mc_batch_add_bulk(db.h, 0, seqs.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p), slot_reads, 0)
        assert added == slot_reads, added
        assert finish() == slot_reads
        return (time.perf_counter() - t) * 1e3

    def file_bytes():
        t = time.perf_counter()
        assert L.mc_batch_add_file_bytes(db.h, 0, raw.ctypes.data, raw.size, 0, 0) == 0
        assert finish() == slot_reads
        return (time.perf_counter() - t) * 1e3

    bulk(); file_bytes()
    a, b = [], []
    for _ in range(reps):
        a.append(bulk()); b.append(file_bytes())
    return {"slot_reads": slot_reads, "slot_bytes": int(raw.size), "mc_batch_add_bulk_ms": spread(a), "mc_batch_add_file_bytes_ms": spread(b)}


def bench_cli(build, db_path, arr, cli_reads, reps):
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "reads.fa")
        arr[:cli_reads].tofile(path)
        for name, args in (("no_map", ["-no-map"]), ("tophits_queryids", ["-tophits", "-queryids"])):
            rows = {"off": [], "on": []}
            for _ in range(reps):
                for sw in ("off", "on"):
                    env = {k: v for k, v in os.environ.items() if k != "MCQ_PARSE_DEVICE"}
                    env["MCQ_PROFILE"] = "1"
                    if sw == "on":
                        env["MCQ_PARSE_DEVICE"] = "1"
                    t = time.perf_counter()
                    r = subprocess.run([build.MCQ, "query", db_path, path] + args + ["-out", os.path.join(tmp, "out.txt")], capture_output=True, text=True, env=env, timeout=1200)
                    wall = (time.perf_counter() - t) * 1e3
                    assert r.returncode == 0, r.stderr[-2000:]
                    m = re.search(r"total ([\d.e+-]+) ms; summed over (\d+) workers: parse\+add ([\d.e+-]+) ms, submit ([\d.e+-]+) ms, wait ([\d.e+-]+) ms", r.stderr)
                    p = re.search(r"reads parsed on the device: (\d+) batches, (\d+) bytes, (\d+) records, (\d+) batches parsed on the host", r.stderr)
                    rows[sw].append({"wall_ms": wall, "job_ms": float(m.group(1)), "workers": int(m.group(2)), "parse_add_ms_summed": float(m.group(3)),
                                     "submit_ms_summed": float(m.group(4)), "wait_ms_summed": float(m.group(5)),
                                     "device_batches": int(p.group(1)) if p else 0, "host_batches": int(p.group(4)) if p else None})
            out[name] = {sw: {"job_ms": spread([x["job_ms"] for x in v]), "parse_add_ms_summed": spread([x["parse_add_ms_summed"] for x in v]),
                              "submit_ms_summed": spread([x["submit_ms_summed"] for x in v]), "runs": v} for sw, v in rows.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--db", required=True)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--slot-reads", type=int, default=65536)
    ap.add_argument("--cli-reads", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cli-reps", type=int, default=3)
    ap.add_argument("--commit", default=None, help="recorded as it is (where the tree is not a git checkout)")
    a = ap.parse_args()
    import torch
    from metacache_amd import api, build
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
        except Exception:
            commit = "unknown"
    meta = {"date": datetime.datetime.now(datetime.timezone.utc).isoformat(timespec="seconds"), "commit": commit, "device": torch.cuda.get_device_name(0),
            "tile": api.parse_tile(), "reps": a.reps}
    os.makedirs(a.out_dir, exist_ok=True)
    db = api.Database.open(a.db, max_candidates=2, slot_max_queries=a.slot_reads, slot_max_chars=a.slot_reads * 330 + 64)
    try:
        for kind in ("fasta", "fastq"):
            arr, head = synthetic(a.reads, kind == "fastq")
            res = dict(meta, kind=kind, kernels=bench_kernels(db, api, torch, arr, a.reps), slot=bench_slot(db, api, arr, head, a.slot_reads, a.reps))
            if kind == "fasta" and a.cli_reads:
                res["cli"] = bench_cli(build, a.db, arr, min(a.cli_reads, a.reads), a.cli_reps)
            with open(os.path.join(a.out_dir, f"parse_{kind}.json"), "w") as f:
                json.dump(res, f, indent=1)
            print(json.dumps({k: res[k] for k in ("kind", "kernels", "slot")}), flush=True)
            if "cli" in res:
                print(json.dumps({n: {sw: {"job_ms": v[sw]["job_ms"], "parse_add": v[sw]["parse_add_ms_summed"]} for sw in v} for n, v in res["cli"].items()}), flush=True)
            del arr
    finally:
        db.close()


if __name__ == "__main__":
    main()
