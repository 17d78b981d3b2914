#!/usr/bin/env python3
"""Measures the device inflate (inflate.hip) on a seeded synthetic FASTQ file of --reads (10^7) reads of 150 bp, compressed
as BGZF at level 6 in members of 65 280 bytes (bgzip's size), by --procs processes.

 (a) mc_inflate_blocks alone, on bytes and rows that are resident on the device, between events: median, minimum and maximum of --reps (7)
     calls after a warm-up; bytes in and bytes out per second.  Decode and CRC are one kernel, so a kernel trace shows one line for both.
 (b) mc_inflate_blocks(MC_INFLATE_HOST) -- index, H2D, kernels and D2H inside the clock -- against the loop `mcq` runs without the
     switch: gzread on one thread into a buffer that grows by doubling (tools/gzread_loop.cpp).  The two alternate in one process.
 (c) `mcq query -no-map` on the file, MCQ_INFLATE_DEVICE unset and set, alternating, --cli-reps (3) runs each: wall time and the `index`
     time of MCQ_PROFILE (the time until the producer has its last batch: with one compressed file nothing goes out before it is inflated).
The device's output is checked against the CRC-32 of every generated piece before anything is timed.

Usage:  python tools/inflate_bench.py --db tests/golden/toy32 [--out profiles/inflate.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import datetime
import json
import multiprocessing
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
PAYLOAD = 65280


RECORD = 15 + 150 + 1 + 2 + 150 + 1                                  # bytes of one generated read


def plain_records(args):
    """records [first, first + n) of the seeded file, as FASTQ text (tools/input_device_bench.py measures on the same file)"""
    first, n, seed = args
    rng = np.random.default_rng([seed, first])
    L = 150
    head = np.frombuffer(b"@read000000000\n", dtype=np.uint8)
    a = np.empty((n, len(head) + L + 1 + 2 + L + 1), dtype=np.uint8)
    a[:, :len(head)] = head
    ids = np.arange(first, first + n, dtype=np.int64)
    for k in range(9):
        a[:, 5 + k] = 48 + (ids // 10 ** (8 - k)) % 10
    at = len(head)
    a[:, at:at + L] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n, L), dtype=np.uint8)]
    a[:, at + L] = 10
    a[:, at + L + 1] = ord("+")
    a[:, at + L + 2] = 10
    a[:, at + L + 3:at + 2 * L + 3] = np.frombuffer(b"FFFFFFFFFFFF:::,,#", dtype=np.uint8)[rng.integers(0, 18, (n, L), dtype=np.uint8)]
    a[:, -1] = 10
    return a.tobytes()


def piece(args):
    """records [first, first + n) as BGZF members -> (compressed bytes, plain length, plain crc32, members)"""
    import inflate_cases
    plain = plain_records(args)
    members = [inflate_cases.bgzf_block(plain[i:i + PAYLOAD], 6) for i in range(0, len(plain), PAYLOAD)]
    return b"".join(members), len(plain), zlib.crc32(plain), len(members)


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def gzread_lib(tmp):
    so = os.path.join(tmp, "libgzread_loop.so")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-fPIC", "-shared", os.path.join(ROOT, "tools", "gzread_loop.cpp"), "-o", so, "-lz"])
    L = C.CDLL(so)
    L.gzread_loop.argtypes = [C.c_char_p, C.POINTER(C.c_uint64)]
    L.gzread_loop.restype = C.c_double
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--db", default=os.path.join(ROOT, "tests", "golden", "toy32"))
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cli-reps", type=int, default=3)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inflate.json"))
    o = ap.parse_args()
    import torch
    from metacache_amd import api, build

    t0 = time.time()
    per = 100_000
    jobs = [(f, min(per, o.reads - f), 1) for f in range(0, o.reads, per)]
    with multiprocessing.get_context("spawn").Pool(o.procs) as pool:
        pieces = pool.map(piece, jobs)
    data = b"".join(p[0] for p in pieces) + __import__("inflate_cases").EOF_BLOCK
    plain_bytes = sum(p[1] for p in pieces)
    res = {"date": datetime.datetime.now().isoformat(timespec="seconds"), "device": torch.cuda.get_device_name(0), "reads": o.reads, "level": 6,
           "bytes_in": len(data), "bytes_out": plain_bytes, "members": sum(p[3] for p in pieces) + 1, "generate_s": round(time.time() - t0, 1)}
    print(json.dumps(res), flush=True)

    db = api.Database.open(o.db, max_candidates=2)
    dev = torch.device("cuda", 0)
    t = time.perf_counter()
    blocks, out_bytes, verdict, _ = api.bgzf_index(data)
    res["index_ms"] = (time.perf_counter() - t) * 1e3
    assert verdict == api.BGZF_OK and out_bytes == plain_bytes
    # ---- (a) resident bytes
    host = np.frombuffer(data, dtype=np.uint8)
    dbytes = torch.zeros((len(data) + 31) // 16 * 16, dtype=torch.uint8, device=dev)
    dbytes[:len(data)] = torch.from_numpy(host.copy())
    drows = torch.from_numpy(blocks.view(np.uint8).copy()).to(dev)
    dout = torch.zeros(out_bytes + 16, dtype=torch.uint8, device=dev)
    dstatus = torch.zeros(4, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=dev)

    def call():
        db.inflate_device(dbytes.data_ptr(), len(data), drows.data_ptr(), len(blocks), dout.data_ptr(), out_bytes, dstatus.data_ptr(), stream=s.cuda_stream)

    call()
    s.synchronize()
    assert [int(x) for x in dstatus.cpu()] == [0, 0, 0, out_bytes], dstatus
    got = dout.cpu().numpy()
    at = 0
    for _, n, crc, _ in pieces:                          # the device's bytes are the generated ones
        assert zlib.crc32(got[at:at + n]) == crc
        at += n
    del got
    ms = []
    for _ in range(o.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        call()
        e1.record(s)
        s.synchronize()
        ms.append(e0.elapsed_time(e1))
    a = spread(ms)
    res["a_device_ms"] = a
    res["a_gb_in_per_s"] = len(data) / a["median"] / 1e6
    res["a_gb_out_per_s"] = out_bytes / a["median"] / 1e6
    print(json.dumps({k: res[k] for k in ("a_device_ms", "a_gb_in_per_s", "a_gb_out_per_s")}), flush=True)
    del dbytes, dout
    # ---- (b) the host form against the gzread loop
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "reads.fq.gz")
        with open(path, "wb") as f:
            f.write(data)
        G = gzread_lib(tmp)
        hostform, loop = [], []
        db.inflate_raw(data, blocks)     # warm-up: the staging buffers are made
        for _ in range(o.reps):
            t = time.perf_counter()
            rows, ob, _, _ = api.bgzf_index(data)
            out, st = db.inflate_raw(data, rows, ob)
            hostform.append((time.perf_counter() - t) * 1e3)
            assert int(st[0]) == 0
            n = C.c_uint64()
            loop.append(G.gzread_loop(path.encode(), C.byref(n)) * 1e3)
            assert n.value == out_bytes
        res["b_host_form_ms"] = spread(hostform)
        res["b_gzread_loop_ms"] = spread(loop)
        res["b_note"] = "host form: index + numpy output allocation + H2D + kernels + D2H; gzread: one thread, buffer grown by doubling"
        print(json.dumps({k: res[k] for k in ("b_host_form_ms", "b_gzread_loop_ms")}), flush=True)
        db.close()
        # ---- (c) mcq
        runs = {"unset": [], "set": []}
        index = {"unset": [], "set": []}
        env0 = {k: v for k, v in os.environ.items() if not k.startswith("MCQ_")}
        env0["MCQ_PROFILE"] = "1"
        for _ in range(o.cli_reps):
            for which in ("unset", "set"):
                env = dict(env0)
                if which == "set":
                    env["MCQ_INFLATE_DEVICE"] = "1"
                t = time.perf_counter()
                r = subprocess.run([build.MCQ, "query", o.db, path, "-no-map", "-out", os.path.join(tmp, "out.txt")], env=env, capture_output=True, text=True)
                runs[which].append((time.perf_counter() - t) * 1e3)
                assert r.returncode == 0, r.stderr
                m = re.search(r"mcq profile: index ([0-9.e+]+) ms, total ([0-9.e+]+) ms", r.stderr)
                index[which].append(float(m.group(1)))
                if which == "set":
                    assert "1 files, " in r.stderr and "0 files left to the host" in r.stderr, r.stderr
        res["c_mcq_wall_ms"] = {k: spread(v) for k, v in runs.items()}
        res["c_mcq_index_ms"] = {k: spread(v) for k, v in index.items()}
    print(json.dumps(res, indent=1))
    if o.out:
        with open(o.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
