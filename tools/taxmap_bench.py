#!/usr/bin/env python3
"""Measures the ranking pass over an accession2taxid table (taxmap.hip) on a seeded synthetic table of --rows (10^7) rows
"RR0000000 RR0000000.1 <taxid> <gi>" of 40 bytes each.  A share --hit-share (0.01) of the accessions are target names; one target has no
row, so every run reads the whole table (the pass would stop where no name is wanted).

 (a) the library, for every name count of --names (10^4, 10^5, 10^6): the file read into memory, its upload from pinned memory, and
     mc_taxmap_add on the resident bytes in pieces of --piece-mb (256), the two kernel groups apart (mc_timing_get: "taxmap_validate",
     "taxmap_match"): the first round is kept apart, then the median, minimum and maximum of --reps (5) rounds;
 (b) `mcq build` of --cli-names (10^4) targets of 130 bp with the table as -taxpostmap, MCQ_TAXMAP_DEVICE unset and set, alternating,
     --cli-reps (2) runs each after a first pair that is kept apart: the ranking pass as mcq's own "ranking pass" line under MCQ_PROFILE
     times it, and the device step's line.  The run with the switch unset is the host loop as it always was.

Usage:  python tools/taxmap_bench.py [--rows 1000000] [--names 10000,100000] [--out-dir profiles]
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

ROW = 40


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def digits(arr, col, width, values):
    for k in range(width):
        arr[:, col + k] = 48 + (values // 10 ** (width - 1 - k)) % 10


def synthetic(rows: int, names: int, share: float, seed: int):
    """-> the table's bytes (a first line and `rows` rows) and the ascending target names.  Accession ids are drawn evenly from
    names / share ids; the names are every (1 / share)-th id, and the rows that would name the LAST name name its neighbour instead."""
    rng = np.random.default_rng(seed)
    stride = max(2, min(int(round(1.0 / share)), (10 ** 7 - 1) // names))     # (seven digits of accession ids)
    space = names * stride
    assert space < 10 ** 7
    ids = rng.integers(0, space, rows, dtype=np.int64)
    ids[ids == (names - 1) * stride] += 1
    arr = np.empty((rows, ROW), dtype=np.uint8)
    arr[:, 0] = arr[:, 1] = arr[:, 10] = arr[:, 11] = ord("R")                 # (two letters: what the sequence id pattern of `build` asks for)
    arr[:, 9] = arr[:, 21] = arr[:, 29] = 9
    arr[:, 19] = ord("."); arr[:, 20] = ord("1"); arr[:, 39] = 10
    digits(arr, 2, 7, ids); digits(arr, 12, 7, ids)
    digits(arr, 22, 7, rng.integers(1, 10 ** 7, rows, dtype=np.int64))
    digits(arr, 30, 9, np.arange(rows, dtype=np.int64) % 10 ** 9)
    return b"accession\taccession.version\ttaxid\tgi\n" + arr.tobytes(), [b"RR%07d.1" % (i * stride) for i in range(names)], 1.0 / stride


def pieces_of(n: int, first: int, limit: int):
    """rows are of one size: pieces of whole rows"""
    per = max(ROW, limit // ROW * ROW)
    return [(b, min(n, b + per)) for b in range(first, n, per)]


def bench_library(api, torch, path, names, piece, reps):
    dev = torch.device("cuda", 0)
    m = api.TaxonMapper()
    lib = api.lib()
    lib.mc_timing_enable(m.h, 1)
    import ctypes as C

    def timing(name):
        ms, cnt = C.c_double(), C.c_uint64()
        lib.mc_timing_get(m.h, name.encode(), C.byref(ms), C.byref(cnt))
        return ms.value

    stream = torch.cuda.Stream(device=dev)
    rounds = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        with open(path, "rb") as f:
            data = f.read()
        read_s = time.perf_counter() - t0
        first = data.index(b"\n") + 1
        m.begin(names)
        lib.mc_timing_reset(m.h)
        h2d = add = 0.0
        status = None
        for b, e in pieces_of(len(data), first, piece):
            host = torch.from_numpy(np.frombuffer(data, dtype=np.uint8)[b:e].copy()).pin_memory()
            d = torch.empty(e - b, dtype=torch.uint8, device=dev)
            ws = torch.empty(api.taxmap_scratch_bytes(e - b), dtype=torch.uint8, device=dev)
            st = torch.zeros(8, dtype=torch.int64, device=dev)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                ev[0].record(stream)
                d.copy_(host, non_blocking=True)
                ev[1].record(stream)
                ev[2].record(stream)
                m.add_device(d.data_ptr(), e - b, status_ptr=st.data_ptr(), workspace_ptr=ws.data_ptr(), workspace_bytes=ws.numel(), stream=stream.cuda_stream)
                ev[3].record(stream)
            stream.synchronize()
            h2d += ev[0].elapsed_time(ev[1]); add += ev[2].elapsed_time(ev[3])
            status = [int(x) for x in st.cpu().numpy()]
            assert status[5] == api.TAXMAP_OK, status
        _, _, remaining = m.result()
        rounds.append({"read_s": read_s, "h2d_ms": h2d, "add_ms": add, "validate_ms": timing("taxmap_validate"), "match_ms": timing("taxmap_match"),
                       "remaining": remaining, "stats": m.stats()})
    m.close()
    out = {"names": len(names), "first_round": rounds[0], "remaining": rounds[-1]["remaining"], "stats_last_round": rounds[-1]["stats"]}
    for k in ("read_s", "h2d_ms", "add_ms", "validate_ms", "match_ms"):
        out[k] = spread([r[k] for r in rounds[1:]])
    return out


def bench_cli(table, names, reps, tmp):
    from metacache_amd import build
    fa = os.path.join(tmp, "targets.fa")
    rng = np.random.default_rng(7)
    with open(fa, "wb") as f:
        for n in names:
            f.write(b">" + n + b" synthetic\n" + bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 130)) + b"\n")
    runs = {"host": {}, "device": {"MCQ_TAXMAP_DEVICE": "1"}}
    out = {k: {"pass_s": [], "wall_s": [], "stderr": []} for k in runs}
    for rep in range(reps + 1):
        for name, extra in runs.items():
            env = dict(os.environ, MCQ_PROFILE="1")
            env.pop("MCQ_TAXMAP_DEVICE", None)
            env.update(extra)
            t0 = time.perf_counter()
            r = subprocess.run([build.MCQ, "build", os.path.join(tmp, "db_" + name), fa, "-taxpostmap", table, "-silent"], capture_output=True, text=True, env=env)
            wall = time.perf_counter() - t0
            if r.returncode != 0:
                raise RuntimeError(f"{name}: {r.stderr[-2000:]}")
            lines = [l for l in r.stderr.split("\n") if "ranking pass" in l or "targets ranked" in l]
            secs = [float(x) for l in lines for x in re.findall(r"ranking pass ([0-9.e+-]+) s", l)]
            assert len(secs) == 1 and (("on the " + name) in " ".join(lines)), r.stderr[-2000:]
            out[name]["pass_s"].append(secs[0]); out[name]["wall_s"].append(wall); out[name]["stderr"] = lines
    with open(os.path.join(tmp, "db_host.meta"), "rb") as a, open(os.path.join(tmp, "db_device.meta"), "rb") as b:
        same = a.read() == b.read()
    return {"targets": len(names), "same_meta_file": same,
            **{k: {"pass_s_first": v["pass_s"][0], "pass_s": spread(v["pass_s"][1:]), "wall_s": spread(v["wall_s"][1:]), "stderr": v["stderr"]} for k, v in out.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--names", default="10000,100000,1000000")
    ap.add_argument("--cli-names", type=int, default=10_000)
    ap.add_argument("--hit-share", type=float, default=0.01)
    ap.add_argument("--piece-mb", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cli-reps", type=int, default=2)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()

    import torch
    from metacache_amd import api
    record = {"tool": "taxmap_bench", "date": datetime.datetime.now().isoformat(timespec="seconds"), "rows": a.rows, "row_bytes": ROW, "hit_share": a.hit_share,
              "piece_mb": a.piece_mb, "reps": a.reps, "cli_reps": a.cli_reps, "device": torch.cuda.get_device_name(0), "library": []}
    with tempfile.TemporaryDirectory() as tmp:
        table = os.path.join(tmp, "synthetic.accession2taxid")
        for n in [int(x) for x in a.names.split(",") if x]:
            data, names, share = synthetic(a.rows, n, a.hit_share, seed=n)          # (10^6 names: the seven-digit id space raises the share)
            with open(table, "wb") as f:
                f.write(data)
            rec = bench_library(api, torch, table, names, a.piece_mb << 20, a.reps)
            rec["hit_share"] = share
            record["library"].append(rec)
        if a.cli_reps >= 0 and a.cli_names:
            data, names, _ = synthetic(a.rows, a.cli_names, a.hit_share, seed=a.cli_names)
            with open(table, "wb") as f:
                f.write(data)
            del data
            record["cli"] = bench_cli(table, names, a.cli_reps, tmp)
    os.makedirs(a.out_dir, exist_ok=True)
    out = os.path.join(a.out_dir, f"taxmap_bench_{a.rows}.json")
    with open(out, "w") as fh:
        json.dump(record, fh, indent=1)
    print(json.dumps(record))
    print("written to", out, file=sys.stderr)


if __name__ == "__main__":
    main()
