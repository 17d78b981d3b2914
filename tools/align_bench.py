#!/usr/bin/env python3
"""Measures mc_align_semiglobal and `mcq query -align` (a record, not a gate; bench.py does not know the option).

  short   --short-problems (10^6) reads of 150 bp against subjects of 240 - 350 characters around their origin, 2 % substitutions
  long    --long-problems (2 000) reads of 5 kbp against subjects of 5 127 - 5 350 characters
          per set: problems/s and cell updates/s (read 1's matrix cells; a problem without a mate is two or three passes over them),
          kernel-only (HIP events around the launches, mc_align_stats) and through the host call, median of --reps calls after a warm-up
  cli     the reference program (oracle/_ref/metacache_u32, where it was built) and mcq on the same box, database and reads --
          tests/golden/build_reads.fa replicated to >= --cli-reads (10^5) reads, -threads 16: query-phase time as each program prints it
          and the process's wall time, with and without -align.  The condition of the -align issue: mcq -align below the reference -align.

Usage:  python tools/align_bench.py [--out profiles/align_bench.json]
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
GOLD = os.path.join(ROOT, "tests", "golden")
REF = os.path.join(ROOT, "oracle", "_ref", "metacache_u32")
FILES = ["build_in/genomes/GCF_000001111.1_ASM111v1_genomic.fna", "build_in/genomes/mixed.fa", "build_in/genomes/assembly_summary.txt",
         "build_in/genomes/more.fa.gz", "build_in/genomes/sub"]
TAX = ["-taxonomy", "build_in/taxonomy"]


def problems(rng, n, read_len, sub_lo, sub_hi):
    """packed reads and subjects cut from one random genome: (chars, offsets) twice"""
    genome = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=8_000_000)
    sl = rng.integers(sub_lo, sub_hi + 1, size=n)
    sp = rng.integers(0, genome.size - sub_hi - 1, size=n)
    so = np.zeros(n + 1, dtype=np.uint64); so[1:] = np.cumsum(sl)
    rp = sp + rng.integers(0, sl - read_len + 1)
    ro = (np.arange(n + 1, dtype=np.uint64) * np.uint64(read_len))
    sc = np.empty(int(so[-1]), dtype=np.uint8)
    rc = np.empty(n * read_len, dtype=np.uint8)
    step = max(1, 20_000_000 // sub_hi)                             # (index arrays of 20 M entries at a time)
    for a in range(0, n, step):
        b = min(n, a + step)
        lo, hi = int(so[a]), int(so[b])
        within = np.arange(hi - lo, dtype=np.int64) - np.repeat(so[a:b].astype(np.int64) - lo, sl[a:b])
        sc[lo:hi] = genome[np.repeat(sp[a:b], sl[a:b]) + within]
        rc[a * read_len:b * read_len] = genome[(rp[a:b, None] + np.arange(read_len)[None, :]).ravel()]
    mut = rng.random(rc.size) < 0.02
    rc[mut] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(mut.sum()))
    return np.append(rc, np.uint8(0)), ro, np.append(sc, np.uint8(0)), so


def measure(A, n, read_len, sub_lo, sub_hi, reps):
    rc, ro, sc, so = problems(np.random.default_rng(5), n, read_len, sub_lo, sub_hi)
    cells = float(((ro[1:] - ro[:-1]) * (so[1:] - so[:-1])).sum())
    A.align_packed(rc, ro, sc, so)                                  # warm-up: allocations, code objects
    host, kern, fwd = [], [], 0
    for _ in range(reps):
        k0 = A.stats()[2]
        t0 = time.perf_counter()
        raw, rev, _, _ = A.align_packed(rc, ro, sc, so)
        host.append(time.perf_counter() - t0)
        kern.append((A.stats()[2] - k0) / 1e9)
        fwd = int((rev == 0).sum())
    h, k = float(np.median(host)), float(np.median(kern))
    return {"problems": n, "read_len": read_len, "subject_len": [sub_lo, sub_hi], "matrix_cells": cells, "shown_forward": fwd, "reps": reps,
            "host_call_s": h, "kernel_s": k, "problems_per_s_host": n / h, "problems_per_s_kernel": n / k,
            "cell_updates_per_s_host": cells / h, "cell_updates_per_s_kernel": cells / k, "sub_batches_per_call": None}


def cli(n_reads, threads):
    from metacache_amd import build
    if not os.path.exists(REF):
        return {"skipped": "oracle/_ref/metacache_u32 is not built here"}
    out = {"threads": threads}
    with tempfile.TemporaryDirectory() as tmp:
        recs = open(os.path.join(GOLD, "build_reads.fa")).read().strip().split("\n>")
        recs = [r.lstrip(">") for r in recs]
        times = (n_reads + len(recs) - 1) // len(recs)
        reads = os.path.join(tmp, "reads.fa")
        with open(reads, "w") as f:
            for t in range(times):
                for r in recs:
                    h, s = r.split("\n", 1)
                    f.write(f">{h.split(' ')[0]}_{t}\n{s}\n")
        out["reads"] = times * len(recs)
        db = os.path.join(tmp, "db")
        subprocess.run([REF, "build", db] + FILES + TAX + ["-threads", "1"], cwd=GOLD, check=True, capture_output=True, timeout=600)
        for prog, exe in (("reference", REF), ("mcq", build.MCQ)):
            for tag, extra in (("plain", []), ("align", ["-align"])):
                res = os.path.join(tmp, f"{prog}_{tag}.txt")
                t0 = time.perf_counter()
                r = subprocess.run([exe, "query", db, reads] + extra + ["-threads", str(threads), "-out", res], cwd=GOLD, capture_output=True, text=True, timeout=1500)
                wall = time.perf_counter() - t0
                if r.returncode != 0:
                    out[f"{prog}_{tag}"] = {"failed": r.stderr[-300:]}
                    continue
                txt = open(res).read()
                m = re.search(r"^# time:    (\d+) ms", txt, re.M)
                out[f"{prog}_{tag}"] = {"process_wall_s": wall, "query_phase_ms": int(m.group(1)) if m else None,
                                        "alignments": txt.count("\n#   score  "), "output_bytes": len(txt)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_bench.json"))
    ap.add_argument("--short-problems", type=int, default=1_000_000)
    ap.add_argument("--long-problems", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cli-reads", type=int, default=100_000)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--scratch-mb", type=int, default=0, help="mc_set_tuning align_scratch_mb (0: the library's default, 512)")
    ap.add_argument("--commit", default=None, help="recorded as it is (where the tree is not a git checkout)")
    a = ap.parse_args()
    from metacache_amd import api
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
        except OSError:
            commit = None
    res = {"date": datetime.datetime.now().isoformat(timespec="seconds"), "commit": commit, "scratch_mb": a.scratch_mb or 512}
    A = api.Aligner()
    try:
        if a.scratch_mb:
            A.set_tuning("align_scratch_mb", a.scratch_mb)
        for name, n, rl, lo, hi in (("short", a.short_problems, 150, 240, 350), ("long", a.long_problems, 5000, 5127, 5350)):
            if n > 0:
                s0 = A.stats()[3]
                res[name] = measure(A, n, rl, lo, hi, a.reps)
                res[name]["sub_batches_per_call"] = (A.stats()[3] - s0) / (a.reps + 1)
                print(name, json.dumps(res[name]), flush=True)
    finally:
        A.close()
    if a.cli_reads > 0:
        res["cli"] = cli(a.cli_reads, a.threads)
        print("cli", json.dumps(res["cli"]), flush=True)
        c = res["cli"]
        if "mcq_align" in c and "reference_align" in c and "query_phase_ms" in c["mcq_align"] and "query_phase_ms" in c["reference_align"]:
            res["mcq_align_faster_than_reference_align"] = bool(c["mcq_align"]["process_wall_s"] < c["reference_align"]["process_wall_s"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
