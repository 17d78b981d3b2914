#!/usr/bin/env python3
"""Golden vectors for `info <db> statistics | featurecounts | featuremap` (the topics that describe the table's content): stdout of
the reference on the toy databases.  Runs only in the build container (oracle/_ref).  Writes tests/golden/table_info_expected.json.gz
(statistics, featurecounts) and tests/golden/table_info_maps_expected.json.gz (featuremap; a file of its own, so that both stay below
the size a committed file may have) -- recorded output only.   python tests/golden/make_golden_table_info.py"""
import gzip
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
DBS = {"toy32": "metacache_u32", "toy16": "metacache_u16", "toy32p2": "metacache_u32", "toy32p4": "metacache_u32"}
CASES = {}
for db, binary in DBS.items():
    CASES[f"statistics_{db}"] = (binary, [db, "statistics"])
    CASES[f"featurecounts_{db}"] = (binary, [db, "featurecounts"])
    if db != "toy32p4":
        CASES[f"featuremap_{db}"] = (binary, [db, "featuremap"])


def main():
    out = {}
    for name, (binary, args) in CASES.items():
        ref = os.path.join(ROOT, "oracle", "_ref", binary)
        if not os.path.exists(ref):
            sys.exit("oracle/_ref is missing: run `make -C oracle ref` first")
        r = subprocess.run([ref, "info"] + args, cwd=HERE, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            sys.exit(r.stderr)
        out[name] = {"args": args, "stdout": r.stdout.split("\n")}
    for fname, keep in (("table_info_expected.json.gz", lambda k: not k.startswith("featuremap_")),
                        ("table_info_maps_expected.json.gz", lambda k: k.startswith("featuremap_"))):
        path = os.path.join(HERE, fname)
        with open(path, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", compresslevel=9, mtime=0) as f:
            f.write(json.dumps({k: v for k, v in out.items() if keep(k)}).encode())
        print(fname, os.path.getsize(path), "bytes")
    print({k: len(v["stdout"]) for k, v in out.items()})


if __name__ == "__main__":
    main()
