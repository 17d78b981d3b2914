#!/usr/bin/env python3
"""Measures `mcq build` with MCQ_BUILD_PARSE_DEVICE unset and set (TargetParseStep, mcq_build.h) on seeded synthetic
collections written as multi-line FASTA files (metacache_amd/synth), in two shapes:

  small:  --small-files (1500) files of --small-records (2) records of --small-bp (32 000) bases each -- many files in one piece;
  large:  --large-files (2) files of one record of --large-bp (300 000 000) bases each -- every file larger than a piece, cut on the host.

Per shape the two settings alternate, --reps (3) runs each after a first pair that is kept apart.  Reported per setting: the wall time and
the ingest phase as mcq's own clock gives it ("Added N reference sequences in X s": taxonomy, the file loop and the builders' finish) as
median and range, and for the device setting the profile line with the kernels' time per GB of FASTA.  With --parent-mcq <binary> the
parent commit's `mcq build` runs in the same alternation: the check that the unset path did not move.  The databases of the settings are
compared byte for byte.  No ratio is asserted: the record says what was measured.

Usage:  python tools/build_parse_bench.py [--reps 3] [--parent-mcq path] [--out-dir profiles]
"""
from __future__ import annotations

import argparse
import datetime
import filecmp
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

LINE = re.compile(r"mcq profile: reference sequences parsed on the device: (\d+) mc_parse_targets calls, (\d+) bytes, (\d+) records, (\d+) targets, "
                  r"kernels (\S+) \+ (\S+) ms, (\d+) files, (\d+) files left to the host")


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def collection(tmp, tag, files, records, bp, seed):
    from metacache_amd import synth
    rng = np.random.default_rng(seed)
    paths = []
    for f in range(files):
        path = os.path.join(tmp, f"{tag}_{f:05d}.fa")
        synth.write_fasta(path, [(f"SYN{tag[0].upper()}_{f:06d}{r:02d}.1 synthetic taxid|{1000 + f}|", synth.random_genome(rng, bp)) for r in range(records)], width=80)
        paths.append(path)
    return paths


def bench_shape(tag, paths, settings, reps, tmp):
    nbytes = sum(os.path.getsize(p) for p in paths)
    listing = os.path.join(tmp, tag + "_files")                # (a directory argument: 1500 names need no long command line)
    out = {k: {"wall_s": [], "ingest_s": [], "profile": None} for k in settings}
    for rep in range(reps + 1):
        for name, (exe, extra) in settings.items():
            env = dict(os.environ, MCQ_PROFILE="1")
            env.pop("MCQ_BUILD_PARSE_DEVICE", None)
            env.update(extra)
            t0 = time.perf_counter()
            r = subprocess.run([exe, "build", os.path.join(tmp, f"db_{tag}_{name}"), listing], capture_output=True, text=True, env=env)
            wall = time.perf_counter() - t0
            if r.returncode != 0:
                raise RuntimeError(f"{tag}/{name}: {r.stderr[-2000:]}")
            added = re.search(r"Added (\d+) reference sequences in ([0-9.e+-]+) s", r.stdout)
            assert added, r.stdout[-1000:]
            m = LINE.search(r.stderr)
            assert (m is not None) == ("MCQ_BUILD_PARSE_DEVICE" in extra), r.stderr[-1000:]
            if rep:
                out[name]["wall_s"].append(wall); out[name]["ingest_s"].append(float(added.group(2)))
            out[name]["targets"] = int(added.group(1))
            if m:
                calls, b, recs, tgts, ms0, ms1, on_dev, left = m.groups()
                assert int(left) == 0 and int(b) == nbytes, m.group(0)
                out[name]["profile"] = {"calls": int(calls), "bytes": int(b), "records": int(recs), "targets": int(tgts), "classify_ms": float(ms0), "write_ms": float(ms1),
                                        "files": int(on_dev), "kernels_ms_per_GB": (float(ms0) + float(ms1)) / (nbytes / 1e9)}
    names = list(settings)
    same = all(filecmp.cmp(os.path.join(tmp, f"db_{tag}_{names[0]}{ext}"), os.path.join(tmp, f"db_{tag}_{n}{ext}"), shallow=False) for n in names[1:] for ext in (".meta", ".cache0"))
    return {"files": len(paths), "fasta_bytes": nbytes, "same_database_files": same,
            **{k: {"wall_s": spread(v["wall_s"]), "ingest_s": spread(v["ingest_s"]), "targets": v["targets"], "profile": v["profile"]} for k, v in out.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small-files", type=int, default=1500)
    ap.add_argument("--small-records", type=int, default=2)
    ap.add_argument("--small-bp", type=int, default=32_000)
    ap.add_argument("--large-files", type=int, default=2)
    ap.add_argument("--large-bp", type=int, default=300_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-mcq", default="")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()

    import torch
    from metacache_amd import build
    if not torch.cuda.is_available():
        raise SystemExit("build_parse_bench: no GPU: nothing is measured")
    settings = {"host": (build.MCQ, {}), "device": (build.MCQ, {"MCQ_BUILD_PARSE_DEVICE": "1"})}
    if a.parent_mcq:
        settings["parent"] = (a.parent_mcq, {})
    record = {"tool": "build_parse_bench", "date": datetime.datetime.now().isoformat(timespec="seconds"), "reps": a.reps, "device": torch.cuda.get_device_name(0),
              "host_threads": os.cpu_count(), "parent_mcq": bool(a.parent_mcq), "shapes": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for tag, files, records, bp in (("small", a.small_files, a.small_records, a.small_bp), ("large", a.large_files, 1, a.large_bp)):
            if files <= 0:
                continue
            os.makedirs(os.path.join(tmp, tag + "_files"))
            paths = collection(os.path.join(tmp, tag + "_files"), tag, files, records, bp, seed=files)
            record["shapes"][tag] = bench_shape(tag, paths, settings, a.reps, tmp)
            for p in paths:
                os.remove(p)
    os.makedirs(a.out_dir, exist_ok=True)
    out = os.path.join(a.out_dir, "build_parse_bench.json")
    with open(out, "w") as fh:
        json.dump(record, fh, indent=1)
    print(json.dumps(record))
    print("written to", out, file=sys.stderr)


if __name__ == "__main__":
    main()
