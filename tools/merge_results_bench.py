#!/usr/bin/env python3
"""Measures the device merge (merge_results.hip) on seeded synthetic part files: --files (4) files of --lines (10^7) result
lines each, ids 1 .. lines, lists of 0-2 entries over the species of a taxonomy (--taxonomy: a directory with nodes.dmp).

 (a) mc_merge_results_add per file on bytes that are resident on the device, between HIP events, against the host-to-device copy of the
     same bytes from pinned memory: the first round is kept apart, then the median, minimum and maximum of --reps (5) rounds.  A range
     takes at most 2^31 bytes: a larger file goes in pieces cut at line starts (MC_MERGE_CONTINUE).
 (b) the wall time of `mcq merge -no-map` on the same files with MCQ_MERGE_DEVICE unset and set, alternating, --cli-reps (3) runs each
     after a first run that is kept apart; and, with --parent-mcq, the same command with the mcq of the parent commit (built elsewhere).

Usage:  python tools/merge_results_bench.py [--lines 100000] [--parent-mcq /path/to/parent/bin/mcq] [--out-dir profiles]
"""
from __future__ import annotations

import argparse
import datetime
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HEAD = (b"# Classification will be constrained to ranks from 'species' to 'domain'.\n"
        b"# TABLE_LAYOUT: query_id\t|\tquery_header\t|\ttop_hits\t|\trank:taxname\n")


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def synthetic_file(lines: int, species, seed: int) -> bytes:
    """`lines` result lines with ids 1 .. lines (ten digits, zero-padded) and 0-2 entries each.  The list parts repeat with a period of
    2^16 lines, so a block of 2^16 lines is one template whose id digits are filled in by numpy."""
    rng = np.random.default_rng(seed)
    P = 1 << 16
    parts = []
    for _ in range(P):
        k = int(rng.integers(0, 3))
        t = rng.choice(species, 2, replace=False)
        h = sorted((int(x) for x in rng.integers(1, 60, 2)), reverse=True)
        parts.append(b"" if k == 0 else b"%d:%d" % (t[0], h[0]) if k == 1 else b"%d:%d,%d:%d" % (t[0], h[0], t[1], h[1]))
    rows = [b"0000000000\t|\tr000000000\t|\t" + x + b"\t|\t--\n" for x in parts]
    starts = np.concatenate(([0], np.cumsum([len(r) for r in rows])))
    template = np.frombuffer(b"".join(rows), dtype=np.uint8)
    out = [HEAD]
    for b in range(0, lines, P):
        m = min(P, lines - b)
        arr = template[:starts[m]].copy()
        ids = np.arange(b + 1, b + m + 1, dtype=np.int64)
        for k in range(10):
            arr[starts[:m] + k] = 48 + (ids // 10 ** (9 - k)) % 10
        for k in range(9):
            arr[starts[:m] + 14 + k] = 48 + ((ids - 1) // 10 ** (8 - k)) % 10
        out.append(arr.tobytes())
    return b"".join(out)


def pieces_of(data: bytes, limit: int = 1 << 31):
    out, pos = [], 0
    while pos < len(data):
        end = min(len(data), pos + limit)
        if end < len(data):
            end = data.rindex(b"\n", pos, end) + 1
        out.append((pos, end))
        pos = end
    return out


def bench_device(api, torch, datas, toy, lines, reps):
    ids, lin, rank = toy
    dev = torch.device("cuda", 0)
    m = api.ResultMerger()
    m.set_taxa(lin, rank, ids)
    stream = torch.cuda.Stream(device=dev)
    add_ms, copy_ms, statuses = [], [], None
    for rep in range(reps + 1):
        m.begin(lines + 1, 2, 4)
        row_add, row_copy, sts = [], [], []
        for data in datas:
            t_add = t_copy = 0.0
            for k, (b, e) in enumerate(pieces_of(data)):
                host = torch.from_numpy(np.frombuffer(data, dtype=np.uint8)[b:e].copy()).pin_memory()
                d = torch.empty(e - b, dtype=torch.uint8, device=dev)
                ws = torch.empty(api.merge_results_scratch_bytes(e - b), dtype=torch.uint8, device=dev)
                st = torch.zeros(8, dtype=torch.int64, device=dev)
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                torch.cuda.synchronize()
                with torch.cuda.stream(stream):
                    ev[0].record(stream)
                    d.copy_(host, non_blocking=True)
                    ev[1].record(stream)
                    ev[2].record(stream)
                    m.add_device(d.data_ptr(), e - b, 2, status_ptr=st.data_ptr(), workspace_ptr=ws.data_ptr(), workspace_bytes=ws.numel(),
                                 file_lines=lines, cont=k > 0, stream=stream.cuda_stream)
                    ev[3].record(stream)
                stream.synchronize()
                t_copy += ev[0].elapsed_time(ev[1])
                t_add += ev[2].elapsed_time(ev[3])
                sts.append([int(x) for x in st.cpu().numpy()])
                assert sts[-1][5] == api.MERGE_OK, sts[-1]
            row_add.append(t_add); row_copy.append(t_copy)
        add_ms.append(row_add); copy_ms.append(row_copy)
        statuses = sts
    m.close()
    per_file = []
    for f in range(len(datas)):
        per_file.append({"bytes": len(datas[f]),
                         "add_ms_first": add_ms[0][f], "add_ms": spread([r[f] for r in add_ms[1:]]),
                         "h2d_ms_first": copy_ms[0][f], "h2d_ms": spread([r[f] for r in copy_ms[1:]])})
    return {"per_file": per_file, "status_last_round": statuses}


def bench_cli(paths, taxonomy, reps, parent_mcq):
    from metacache_amd import build
    runs = {"host": (build.MCQ, {}), "device": (build.MCQ, {"MCQ_MERGE_DEVICE": "1"})}
    if parent_mcq:
        runs["parent"] = (parent_mcq, {})
    times = {k: [] for k in runs}
    notes = {}
    for rep in range(reps + 1):
        for name, (exe, extra) in runs.items():
            env = dict(os.environ, MCQ_PROFILE="1")
            env.pop("MCQ_MERGE_DEVICE", None)
            env.update(extra)
            t0 = time.perf_counter()
            r = subprocess.run([exe, "merge"] + paths + ["-taxonomy", taxonomy, "-no-map", "-silent"], capture_output=True, text=True, env=env)
            times[name].append(time.perf_counter() - t0)
            if r.returncode != 0:
                raise RuntimeError(f"{name}: {r.stderr[-2000:]}")
            notes[name] = [l for l in r.stderr.split("\n") if "result files merged" in l]
            notes[name + "_summary"] = [l for l in r.stdout.split("\n") if l.startswith("# ") and ("classified" in l or "species" in l)][:3]
    return {k: {"wall_s_first": v[0], "wall_s": spread(v[1:]), "stderr": notes[k], "summary": notes[k + "_summary"]} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=4)
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cli-reps", type=int, default=3)
    ap.add_argument("--taxonomy", default=os.path.join(ROOT, "tests", "golden", "build_in", "taxonomy"))
    ap.add_argument("--parent-mcq", default="")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--skip-device", action="store_true")
    a = ap.parse_args()

    import merge_results_cases as cases
    import evaluate_ref
    taxa = cases.read_taxonomy(a.taxonomy)
    lin, rank, _ = evaluate_ref.taxon_table(taxa)
    ids = np.array([t[0] for t in taxa], dtype=np.int64)
    species = [int(i) for i, r in zip(ids, rank) if r == 4]
    datas = [synthetic_file(a.lines, species, seed=100 + f) for f in range(a.files)]
    record = {"tool": "merge_results_bench", "date": datetime.datetime.now().isoformat(timespec="seconds"), "files": a.files, "lines": a.lines,
              "bytes": [len(d) for d in datas], "reps": a.reps, "cli_reps": a.cli_reps}
    if not a.skip_device:
        import torch
        from metacache_amd import api
        record["device"] = bench_device(api, torch, datas, (ids, lin, rank), a.lines, a.reps)
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for f, d in enumerate(datas):
            paths.append(os.path.join(tmp, f"part{f}.txt"))
            with open(paths[-1], "wb") as fh:
                fh.write(d)
        record["cli"] = bench_cli(paths, a.taxonomy if a.taxonomy.endswith("/") else a.taxonomy + "/", a.cli_reps, a.parent_mcq)
    os.makedirs(a.out_dir, exist_ok=True)
    out = os.path.join(a.out_dir, f"merge_results_bench_{a.files}x{a.lines}.json")
    with open(out, "w") as fh:
        json.dump(record, fh, indent=1)
    print(json.dumps(record))
    print("written to", out, file=sys.stderr)


if __name__ == "__main__":
    main()
