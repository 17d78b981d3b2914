#!/usr/bin/env python3
"""Golden vectors for `query -align`: what the REFERENCE prints with the option, on databases it built from build_in.

Runs only in the build container (needs oracle/_ref/metacache_u32 = the reference compiled by `make -C oracle ref`), with
cwd = tests/golden, so that the file names stored in the databases are the relative build_in/genomes/... paths the repository holds.
Writes data only, under tests/golden/:

  align_pairs.fq            100 read pairs drawn from the build_in genomes (2 % mutations, some mates reverse-complemented, a few
                            lower-case stretches and N), interleaved
  align_long.fa             12 reads of 600 - 6 000 bp
  align_expected.json.gz    per case: database ("default" / "w64"), options, reads file, and the complete output file of the reference

The reference reads the record BEFORE a target's own (tests/align_ref.py, record rule "reference"); the goldens record that as it is.

Usage:  python tests/golden/make_golden_align.py
"""
from __future__ import annotations

import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import align_ref  # noqa: E402

REF32 = os.path.join(ROOT, "oracle", "_ref", "metacache_u32")
FILES = ["build_in/genomes/GCF_000001111.1_ASM111v1_genomic.fna", "build_in/genomes/mixed.fa", "build_in/genomes/assembly_summary.txt",
         "build_in/genomes/more.fa.gz", "build_in/genomes/sub"]
TAX = ["-taxonomy", "build_in/taxonomy"]
DATABASES = {"default": [], "w64": ["-winlen", "64", "-winstride", "40"]}
# name -> (database, reads file, options, run from another directory)
CASES = {
    "align": ("default", "build_reads.fa", ["-align"], False),
    "align_tophits": ("default", "build_reads.fa", ["-align", "-tophits", "-queryids", "-locations"], False),
    "align_mapped_only": ("default", "build_reads.fa", ["-align", "-mapped-only", "-comment", "%%", "-separator", ";"], False),
    "align_species": ("default", "build_reads.fa", ["-align", "-lowest", "species"], False),
    "align_maxcand": ("default", "build_reads.fa", ["-align", "-maxcand", "4", "-hitdiff", "50"], False),
    "align_pairs": ("default", "align_pairs.fq", ["-pairseq", "-align", "-tophits"], False),
    "align_long": ("default", "align_long.fa", ["-alignment"], False),
    "align_cov": ("default", "build_reads.fa", ["-align", "-cov-percentile", "0.3"], False),
    "align_w64": ("w64", "build_reads.fa", ["-align", "-tophits", "-locations"], False),
    "align_elsewhere": ("default", "build_reads.fa", ["-align", "-tophits"], True),
}


def mutate(rng, g, rate):
    g = g.copy()
    pos = np.nonzero(rng.random(g.size) < rate)[0]
    g[pos] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=pos.size)
    return g


def make_reads():
    rng = np.random.default_rng(20261016)
    pool = []
    for f in ("GCF_000001111.1_ASM111v1_genomic.fna", "mixed.fa", "more.fa.gz", "sub/GCF_000002222.2_other.fa"):
        for _, s in align_ref.read_records(os.path.join(HERE, "build_in", "genomes", f)):
            if len(s) > 7000:
                pool.append(np.frombuffer(s, dtype=np.uint8))
    lines = []
    for i in range(100):
        g = pool[int(rng.integers(len(pool)))]
        l1, l2, ins = int(rng.integers(80, 152)), int(rng.integers(80, 152)), int(rng.integers(200, 420))
        p = int(rng.integers(0, g.size - ins - 160))
        r1 = mutate(rng, g[p:p + l1], 0.02)
        r2 = mutate(rng, g[p + ins - l2 + 150:p + ins + 150], 0.02)
        r1, r2 = bytes(r1), bytes(r2)
        if rng.random() < 0.7:
            r2 = align_ref.reverse_complement(r2)
        if rng.random() < 0.3:
            r1, r2 = align_ref.reverse_complement(r1), align_ref.reverse_complement(r2)
        if i % 9 == 0:
            r1 = r1[:20] + r1[20:50].lower() + r1[50:]
        if i % 13 == 0:
            r2 = r2[:30] + b"NNNN" + r2[34:]
        for k, r in ((1, r1), (2, r2)):
            lines.append(f"@pair{i}/{k}\n{r.decode()}\n+\n{'I' * len(r)}")
    open(os.path.join(HERE, "align_pairs.fq"), "w").write("\n".join(lines) + "\n")
    lines = []
    for i in range(12):
        g = pool[int(rng.integers(len(pool)))]
        n = int(rng.integers(600, 6001))
        p = int(rng.integers(0, g.size - n))
        r = bytes(mutate(rng, g[p:p + n], 0.02))
        if i % 2:
            r = align_ref.reverse_complement(r)
        lines.append(f">long{i} len={n}\n{r.decode()}")
    open(os.path.join(HERE, "align_long.fa"), "w").write("\n".join(lines) + "\n")


def run(cmd, cwd):
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=1800)
    if r.returncode != 0:
        sys.exit(f"FAILED: {' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
    return r


def main():
    if not os.path.exists(REF32):
        sys.exit("oracle/_ref is missing: run `make -C oracle ref` first")
    make_reads()
    out = {"files": FILES, "tax": TAX, "databases": DATABASES, "cases": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for name, extra in DATABASES.items():
            run([REF32, "build", os.path.join(tmp, name)] + FILES + TAX + extra + ["-threads", "1"], HERE)
        other = os.path.join(tmp, "elsewhere")
        os.makedirs(other)
        for name, (db, reads, args, elsewhere) in CASES.items():
            res = os.path.join(tmp, name + ".txt")
            cwd = HERE
            if elsewhere:                                   # every source file is missing from there: no alignment lines
                shutil.copy(os.path.join(HERE, reads), os.path.join(other, reads))
                cwd = other
            run([REF32, "query", os.path.join(tmp, db), reads] + args + ["-threads", "1", "-no-err", "-out", res], cwd)
            out["cases"][name] = {"db": db, "reads": reads, "args": args, "elsewhere": elsewhere, "lines": open(res).read().split("\n")}
    with gzip.GzipFile(os.path.join(HERE, "align_expected.json.gz"), "wb", mtime=0) as f:
        f.write(json.dumps(out).encode())
    print("wrote align_expected.json.gz:", {k: (len(v["lines"]), sum("  score  " in l for l in v["lines"])) for k, v in out["cases"].items()})


if __name__ == "__main__":
    main()
