#!/usr/bin/env python3
"""Measures the device cut and the header packing (parse_cut.hip) on the seeded synthetic FASTQ of tools/inflate_bench.py:
--reads (10^7) reads of 150 bp, plain, resident on the device.

 (a) mc_parse_cut over the whole file in pieces of at most 2^31 bytes (every piece but the last with MC_CUT_OPEN, the next one starting at
     `consumed`, as a caller chains them), between events: median, minimum and maximum of --reps (7) passes after a warm-up pass; bytes read
     over time.  mc_parse_headers behind mc_parse_records on the first --header-bytes (256 MiB) of whole records, the same way.
     The cuts are checked before anything is timed: every batch holds --batch reads of 319 bytes.
 (b) `mcq query -no-map` on the file, plain and as BGZF (level 6, members of 65 280 bytes), --cli-reps (3) runs each of three
     configurations, alternating in one session: the switches unset; MCQ_INFLATE_DEVICE=1 MCQ_PARSE_DEVICE=1 (the best path without
     resident input); MCQ_INPUT_DEVICE=1.  Wall time of the job and the `index` time of MCQ_PROFILE (the time until the producer has its
     last batch).  --cli-reads (default: --reads) reads go into the two files.

Usage:  python tools/input_device_bench.py --db tests/golden/toy32 [--out profiles/input_device.json]
"""
from __future__ import annotations

import argparse
import datetime
import json
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from inflate_bench import RECORD, piece, plain_records                      # the generator of 7j's file: one file for both records


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--db", default=os.path.join(ROOT, "tests", "golden", "toy32"))
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--piece", type=int, default=1 << 31)
    ap.add_argument("--header-bytes", type=int, default=256 << 20)
    ap.add_argument("--cli-reps", type=int, default=3)
    ap.add_argument("--cli-reads", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "input_device.json"))
    o = ap.parse_args()
    import torch
    from metacache_amd import api

    t0 = time.time()
    per = 100_000
    jobs = [(f, min(per, o.reads - f), 1) for f in range(0, o.reads, per)]
    with multiprocessing.get_context("spawn").Pool(o.procs) as pool:
        pieces = pool.map(plain_records, jobs)
    dev = torch.device("cuda", 0)
    total = sum(len(p) for p in pieces)
    dbytes = torch.zeros(total + 64, dtype=torch.uint8, device=dev)
    at = 0
    for p in pieces:
        dbytes[at:at + len(p)] = torch.from_numpy(np.frombuffer(p, dtype=np.uint8).copy()).to(dev)
        at += len(p)
    del pieces
    res = {"date": datetime.datetime.now().isoformat(timespec="seconds"), "device": torch.cuda.get_device_name(0), "reads": o.reads, "bytes": total,
           "batch": o.batch, "piece": o.piece, "generate_s": round(time.time() - t0, 1)}
    print(json.dumps(res), flush=True)

    db = api.Database.open(o.db, max_candidates=2)
    s = torch.cuda.Stream(device=dev)
    capacity = min(o.piece, total) // (RECORD * o.batch) + 2
    cuts = torch.zeros(capacity, dtype=torch.int64, device=dev)
    status = torch.zeros(8, dtype=torch.int64, device=dev)
    wsb = api.parse_cut_scratch_bytes(min(o.piece, total))
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def one_pass(check):
        """the whole file, piece by piece -> (ms between events, calls); the host reads `consumed` between two pieces, outside the events"""
        pos, ms, calls, whole = 0, 0.0, 0, 0
        while pos < total:
            n = min(o.piece, total - pos)
            last = pos + n == total
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            db.parse_cut_device(dbytes.data_ptr() + pos, n, o.batch, cuts_ptr=cuts.data_ptr(), capacity=capacity, status_ptr=status.data_ptr(),
                                workspace_ptr=ws.data_ptr(), workspace_bytes=wsb, open=not last, stream=s.cuda_stream)
            e1.record(s)
            s.synchronize()
            ms += e0.elapsed_time(e1)
            calls += 1
            st = [int(x) for x in status.cpu()]
            assert st[4] == api.PARSE_OK and st[2] > 0, st
            if check:
                c = cuts.cpu().numpy()[:st[1] + 1]
                assert st[2] % RECORD == 0 and st[0] == st[2] // RECORD and st[6] == min(o.batch, st[0]) * RECORD, st
                assert np.all(np.diff(c)[:-1] == o.batch * RECORD) and int(c[-1]) == st[2]
            whole += st[0]
            pos += st[2]
        assert whole == o.reads
        return ms, calls

    _, calls = one_pass(True)
    ms = [one_pass(False)[0] for _ in range(o.reps)]
    a = spread(ms)
    res["a_cut_ms"] = a
    res["a_cut_calls_per_pass"] = calls
    res["a_cut_gb_per_s"] = total / a["median"] / 1e6
    print(json.dumps({k: res[k] for k in ("a_cut_ms", "a_cut_calls_per_pass", "a_cut_gb_per_s")}), flush=True)

    # ---- mc_parse_headers behind mc_parse_records
    n = min(o.header_bytes, total) // RECORD * RECORD
    recs = n // RECORD
    z = lambda k, dt: torch.zeros(max(k, 1), dtype=dt, device=dev)
    hdr, qinfo, seq, names = z(2 * recs, torch.int32), z(4 * recs, torch.int32), z(recs * 152 + 16, torch.uint8), z(recs * 14 + 16, torch.uint8)
    name_off, max_win, pstatus = z(recs + 1, torch.int64), z(recs, torch.int32), z(8, torch.int64)
    pwsb = api.parse_scratch_bytes(n)
    pws = z(pwsb, torch.uint8)
    out, out_off, hstatus = z(recs * 14, torch.uint8), z(recs + 1, torch.int64), z(4, torch.int64)
    hwsb = api.parse_headers_scratch_bytes(recs)
    hws = z(hwsb, torch.uint8)
    torch.cuda.synchronize()
    db.parse_device(dbytes.data_ptr(), n, hdr_ptr=hdr.data_ptr(), qinfo_ptr=qinfo.data_ptr(), seq_ptr=seq.data_ptr(), seq_capacity=recs * 152 + 16, names_ptr=names.data_ptr(),
                    names_capacity=recs * 14 + 16, name_off_ptr=name_off.data_ptr(), max_win_ptr=max_win.data_ptr(), status_ptr=pstatus.data_ptr(), max_records=recs,
                    workspace_ptr=pws.data_ptr(), workspace_bytes=pwsb, stream=s.cuda_stream)

    def heads():
        db.parse_headers_device(dbytes.data_ptr(), n, hdr_ptr=hdr.data_ptr(), parse_status_ptr=pstatus.data_ptr(), max_records=recs, out_ptr=out.data_ptr(),
                                out_capacity=recs * 14, out_off_ptr=out_off.data_ptr(), status_ptr=hstatus.data_ptr(), workspace_ptr=hws.data_ptr(), workspace_bytes=hwsb,
                                stream=s.cuda_stream)

    heads()
    s.synchronize()
    assert [int(x) for x in hstatus.cpu()] == [recs, recs * 13, 0, 0], hstatus
    assert out.cpu().numpy()[:26].tobytes() == b"read000000000read000000001"
    ms = []
    for _ in range(o.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        heads()
        e1.record(s)
        s.synchronize()
        ms.append(e0.elapsed_time(e1))
    res["a_headers_ms"] = spread(ms)
    res["a_headers_records"] = recs
    res["a_headers_range_bytes"] = n
    db.close()
    del dbytes, hdr, qinfo, seq, names, name_off, max_win, out, out_off, pws, hws, ws, cuts
    torch.cuda.empty_cache()
    # ---- (b) mcq
    import re
    import subprocess
    import tempfile
    from metacache_amd import build
    import inflate_cases
    cli_reads = o.cli_reads or o.reads
    jobs = [(f, min(per, cli_reads - f), 1) for f in range(0, cli_reads, per)]
    configs = {"unset": {}, "inflate+parse": {"MCQ_INFLATE_DEVICE": "1", "MCQ_PARSE_DEVICE": "1"}, "input": {"MCQ_INPUT_DEVICE": "1"}}
    with tempfile.TemporaryDirectory() as tmp:
        paths = {"plain": os.path.join(tmp, "reads.fq"), "bgzf": os.path.join(tmp, "reads.fq.gz")}
        with multiprocessing.get_context("spawn").Pool(o.procs) as pool:
            with open(paths["plain"], "wb") as f:
                for p in pool.imap(plain_records, jobs):
                    f.write(p)
            with open(paths["bgzf"], "wb") as f:
                for p in pool.imap(piece, jobs):
                    f.write(p[0])
                f.write(inflate_cases.EOF_BLOCK)
        env0 = {k: v for k, v in os.environ.items() if not k.startswith("MCQ_")}
        env0["MCQ_PROFILE"] = "1"
        res["b_reads"] = cli_reads
        res["b_bytes"] = {k: os.path.getsize(v) for k, v in paths.items()}
        for kind, path in paths.items():
            wall, index = {k: [] for k in configs}, {k: [] for k in configs}
            for _ in range(o.cli_reps):
                for which, switches in configs.items():
                    t = time.perf_counter()
                    r = subprocess.run([build.MCQ, "query", o.db, path, "-no-map", "-out", os.path.join(tmp, "out.txt")], env={**env0, **switches}, capture_output=True, text=True)
                    wall[which].append((time.perf_counter() - t) * 1e3)
                    assert r.returncode == 0, r.stderr
                    index[which].append(float(re.search(r"mcq profile: index ([0-9.e+]+) ms", r.stderr).group(1)))
                    if which == "input":
                        assert "input resident on the device: 1 files" in r.stderr and "0 files left to the host" in r.stderr, r.stderr
            res["b_mcq_wall_ms_" + kind] = {k: spread(v) for k, v in wall.items()}
            res["b_mcq_index_ms_" + kind] = {k: spread(v) for k, v in index.items()}
            print(json.dumps({k: res[k] for k in ("b_mcq_wall_ms_" + kind, "b_mcq_index_ms_" + kind)}), flush=True)
    res["note"] = "one MI355X, one process per configuration; toy database, one file, synthetic qualities"
    print(json.dumps(res, indent=1))
    if o.out:
        os.makedirs(os.path.dirname(o.out), exist_ok=True)
        with open(o.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
