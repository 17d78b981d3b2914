#!/usr/bin/env python3
"""Measures the device inflate of whole gzip files (mc_inflate_streams, inflate_streams.hip) and `mcq build` with
MCQ_BUILD_PARSE_DEVICE + MCQ_BUILD_INFLATE_DEVICE unset and set, on seeded synthetic collections written as multi-line FASTA files
(metacache_amd/synth) and gzipped at level 6, in two shapes:

  small:  --small-files (1500) files of --small-records (2) records of --small-bp (32 000) bases each -- tools/build_parse_bench.py's
          small shape, 97 MB plain;
  medium: --medium-files (200) files of one record of --medium-bp (5 000 000) bases each -- about 5 MB plain per file.

Per shape:
  * the call on resident bytes: every file one row, mc_inflate_streams (device form) between two events, --call-reps (5) times after one
    call kept apart: ms and GB/s in and out as median [min .. max], beside the longest row's plain size and that row ALONE in a call of
    its own -- which says whether the call waits for one wave;
  * `mcq build` with both switches unset, with both set, and -- with --parent-mcq <binary> -- the parent commit's `mcq build`, alternating,
    --reps (5) runs each after a first round kept apart: wall time and the ingest phase as mcq's own clock gives it ("Added N reference
    sequences in X s") as median [min .. max], and the set run's profile line.  The databases are compared byte for byte.
And once: single rows of --row-mb (1, 4, 16, 64) MB plain, each alone in a call, beside zlib's time for the same file on one host
thread -- the measurement MCQ_BUILD_INFLATE_MAX_MB's default is to be checked against.
No ratio is asserted: the record says what was measured.

Usage:  python tools/build_inflate_bench.py [--reps 5] [--parent-mcq path] [--out-dir profiles]
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
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LINE = re.compile(r"mcq profile: gzip references inflated on the device: (\d+) files, (\d+) bytes in, (\d+) bytes out, (\d+) mc_inflate_streams calls, kernels (\S+) ms, "
                  r"(\d+) gzip files left to the host")


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def fasta_bytes(header, seq, width=80):
    b = seq.tobytes()
    return b">" + header.encode() + b"\n" + b"".join(b[i:i + width] + b"\n" for i in range(0, len(b), width))


def gzip_file(plain):
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    return c.compress(plain) + c.flush()


def collection(tmp, tag, files, records, bp, seed):
    """-> [(path, plain bytes, compressed bytes)]; the files are written gzipped"""
    from metacache_amd import synth
    rng = np.random.default_rng(seed)
    out = []
    for f in range(files):
        plain = b"".join(fasta_bytes(f"SYN{tag[0].upper()}_{f:06d}{r:02d}.1 synthetic taxid|{1000 + f}|", synth.random_genome(rng, bp)) for r in range(records))
        z = gzip_file(plain)
        path = os.path.join(tmp, f"{tag}_{f:05d}.fa.gz")
        with open(path, "wb") as fh:
            fh.write(z)
        out.append((path, len(plain), z))
    return out


def time_call(db, api, torch, files, caps, reps):
    """the device form on resident bytes: -> (ms per call [reps], accepted rows, bytes out)"""
    rows = np.zeros(len(files), dtype=api.gzip_stream_dtype)
    at = out_at = 0
    for i, (z, cap) in enumerate(zip(files, caps)):
        rows[i] = (at, len(z), out_at, cap)
        at += (len(z) + 15) // 16 * 16
        out_at += cap
    data = np.zeros(at + 16, dtype=np.uint8)
    for r, z in zip(rows, files):
        data[int(r["in_off"]):int(r["in_off"]) + len(z)] = np.frombuffer(z, dtype=np.uint8)
    dev = torch.device("cuda", 0)
    d_bytes, d_rows = torch.from_numpy(data).to(dev), torch.from_numpy(rows.view(np.uint8).copy()).to(dev)
    d_out = torch.zeros(out_at + 16, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(16 * len(files), dtype=torch.uint8, device=dev)
    d_st = torch.zeros(4, dtype=torch.int64, device=dev)
    ms = []
    stream = torch.cuda.Stream(device=dev)                  # the events and the call on ONE stream: the events bracket the three launches
    torch.cuda.synchronize()
    for rep in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        db.inflate_streams_device(d_bytes.data_ptr(), at, d_rows.data_ptr(), len(files), d_out.data_ptr(), out_at, d_res.data_ptr(), d_st.data_ptr(), stream=stream.cuda_stream)
        b.record(stream)
        torch.cuda.synchronize()
        if rep:
            ms.append(a.elapsed_time(b))
    st = d_st.cpu().numpy().view(np.uint64)
    assert int(st[0]) == api.INFLATE_OK and int(st[3]) == len(files), st
    return ms, at, out_at


def bench_call(db, api, torch, coll, reps):
    files, caps = [c[2] for c in coll], [c[1] for c in coll]
    ms, nin, nout = time_call(db, api, torch, files, caps, reps)
    k = int(np.argmax(caps))
    one, _, _ = time_call(db, api, torch, [files[k]], [caps[k]], reps)
    s = spread(ms)
    return {"rows": len(files), "bytes_in": nin, "bytes_out": nout, "ms": s, "GBps_in": nin / s["median"] / 1e6, "GBps_out": nout / s["median"] / 1e6,
            "longest_row_plain_bytes": caps[k], "longest_row_alone_ms": spread(one)}


def bench_build(tag, listing, settings, reps, tmp, nfiles):
    out = {k: {"wall_s": [], "ingest_s": [], "profile": None} for k in settings}
    for rep in range(reps + 1):
        for name, (exe, extra) in settings.items():
            env = dict(os.environ, MCQ_PROFILE="1")
            for k in ("MCQ_BUILD_PARSE_DEVICE", "MCQ_BUILD_INFLATE_DEVICE", "MCQ_BUILD_INFLATE_MAX_MB"):
                env.pop(k, None)
            env.update(extra)
            t0 = time.perf_counter()
            r = subprocess.run([exe, "build", os.path.join(tmp, f"db_{tag}_{name}"), listing], capture_output=True, text=True, env=env)
            wall = time.perf_counter() - t0
            if r.returncode != 0:
                raise RuntimeError(f"{tag}/{name}: {r.stderr[-2000:]}")
            added = re.search(r"Added (\d+) reference sequences in ([0-9.e+-]+) s", r.stdout)
            assert added, r.stdout[-1000:]
            m = LINE.search(r.stderr)
            assert (m is not None) == ("MCQ_BUILD_INFLATE_DEVICE" in extra), r.stderr[-1000:]
            if rep:
                out[name]["wall_s"].append(wall); out[name]["ingest_s"].append(float(added.group(2)))
            out[name]["targets"] = int(added.group(1))
            if m:
                files, bin_, bout, calls, ms, left = m.groups()
                assert int(left) == 0 and int(files) == nfiles, m.group(0)
                out[name]["profile"] = {"files": int(files), "bytes_in": int(bin_), "bytes_out": int(bout), "calls": int(calls), "kernels_ms": float(ms)}
    names = list(settings)
    same = all(filecmp.cmp(os.path.join(tmp, f"db_{tag}_{names[0]}{ext}"), os.path.join(tmp, f"db_{tag}_{n}{ext}"), shallow=False) for n in names[1:] for ext in (".meta", ".cache0"))
    return {"same_database_files": same,
            **{k: {"wall_s": spread(v["wall_s"]), "ingest_s": spread(v["ingest_s"]), "targets": v["targets"], "profile": v["profile"]} for k, v in out.items()}}


def bench_rows(db, api, torch, sizes_mb, reps):
    """one row alone in a call, beside zlib on one host thread"""
    from metacache_amd import synth
    rng = np.random.default_rng(77)
    out = []
    for mb in sizes_mb:
        plain = fasta_bytes(f"ROW_{mb}.1 synthetic", synth.random_genome(rng, int(mb * (1 << 20) * 80 / 81)))
        z = gzip_file(plain)
        ms, _, _ = time_call(db, api, torch, [z], [len(plain)], reps)
        host = []
        for _ in range(reps):
            t0 = time.perf_counter()
            got = zlib.decompress(z, 31)
            host.append((time.perf_counter() - t0) * 1e3)
        assert got == plain
        out.append({"plain_bytes": len(plain), "compressed_bytes": len(z), "device_ms": spread(ms), "zlib_ms": spread(host),
                    "device_MBps_out": len(plain) / spread(ms)["median"] / 1e3, "zlib_MBps_out": len(plain) / spread(host)["median"] / 1e3})
        print("row", json.dumps(out[-1]), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small-files", type=int, default=1500)
    ap.add_argument("--small-records", type=int, default=2)
    ap.add_argument("--small-bp", type=int, default=32_000)
    ap.add_argument("--medium-files", type=int, default=200)
    ap.add_argument("--medium-bp", type=int, default=5_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--call-reps", type=int, default=5)
    ap.add_argument("--row-mb", type=float, nargs="*", default=[1, 4, 16, 64])
    ap.add_argument("--parent-mcq", default="")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()

    import torch
    from metacache_amd import api, build
    if not torch.cuda.is_available():
        raise SystemExit("build_inflate_bench: no GPU: nothing is measured")
    both = {"MCQ_BUILD_PARSE_DEVICE": "1", "MCQ_BUILD_INFLATE_DEVICE": "1", "MCQ_BUILD_INFLATE_MAX_MB": "64"}
    settings = {"unset": (build.MCQ, {}), "set": (build.MCQ, both)}
    if a.parent_mcq:
        settings["parent"] = (a.parent_mcq, {})
    record = {"tool": "build_inflate_bench", "date": datetime.datetime.now().isoformat(timespec="seconds"), "reps": a.reps, "call_reps": a.call_reps,
              "device": torch.cuda.get_device_name(0), "host_threads": os.cpu_count(), "parent_mcq": bool(a.parent_mcq), "gzip_level": 6, "shapes": {}}
    db = api.Database.create()
    try:
        with tempfile.TemporaryDirectory() as tmp:
            for tag, files, records, bp in (("small", a.small_files, a.small_records, a.small_bp), ("medium", a.medium_files, 1, a.medium_bp)):
                if files <= 0:
                    continue
                d = os.path.join(tmp, tag + "_files")
                os.makedirs(d)
                coll = collection(d, tag, files, records, bp, seed=files)
                shape = {"files": files, "plain_bytes": sum(c[1] for c in coll), "gzip_bytes": sum(len(c[2]) for c in coll)}
                shape["call"] = bench_call(db, api, torch, coll, a.call_reps)
                print(tag, "call", json.dumps(shape["call"]), file=sys.stderr, flush=True)
                coll = [(c[0], c[1], None) for c in coll]
                shape["build"] = bench_build(tag, d, settings, a.reps, tmp, files)
                print(tag, "build", json.dumps(shape["build"]), file=sys.stderr, flush=True)
                record["shapes"][tag] = shape
                for c in coll:
                    os.remove(c[0])
        record["single_rows"] = bench_rows(db, api, torch, a.row_mb, 3)
    finally:
        db.close()
    os.makedirs(a.out_dir, exist_ok=True)
    out = os.path.join(a.out_dir, "build_inflate_bench.json")
    with open(out, "w") as fh:
        json.dump(record, fh, indent=1)
    print(json.dumps(record))
    print("written to", out, file=sys.stderr)


if __name__ == "__main__":
    main()
