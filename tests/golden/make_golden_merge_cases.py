#!/usr/bin/env python3
"""Golden vectors for the device merge: three small generated part files (tests/merge_results_cases.generated_files: ids with gaps, a
query in one file only, ties, the same taxon with more / as many / fewer hits, an unknown and a negative taxid, an empty list in every
file, a top candidate without a rank) and what the reference's `metacache merge` makes of them.  Runs only in the build container (needs
oracle/_ref/metacache_u32).  Writes data only:

  merge_cases_in/a.txt, b.txt, c.txt       the part files (written at -maxcand 8)
  merge_cases_expected.json.gz             {case: {"files": [...], "args": [...], "lines": [...]}}

Usage:  python tests/golden/make_golden_merge_cases.py
"""
import gzip
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(ROOT, "oracle", "_ref", "metacache_u32")
TAX = "build_in/taxonomy"
sys.path.insert(0, os.path.join(ROOT, "tests"))

ALL = ["merge_cases_in/a.txt", "merge_cases_in/b.txt", "merge_cases_in/c.txt"]
SHOW = ["-tophits", "-queryids", "-taxids"]
CASES = {
    "three_maxcand8": (ALL, ["-maxcand", "8"] + SHOW),
    "three_maxcand1": (ALL, ["-maxcand", "1"] + SHOW),
    "three_default": (ALL, SHOW),
    "a_b_cut": (ALL[:2], ["-maxcand", "8"] + SHOW),
    "b_c_grow": (ALL[1:], ["-maxcand", "4"] + SHOW),
    "a_c_vote": ([ALL[0], ALL[2]], ["-maxcand", "8", "-hitmin", "3", "-hitdiff", "0.5", "-highest", "family"] + SHOW),
    "three_lineage": (ALL, ["-maxcand", "8", "-lineage", "-mapped-only"] + SHOW),
}


def main():
    import merge_results_cases as cases
    if not os.path.exists(REF):
        sys.exit("oracle/_ref is missing: run `make -C oracle ref` first")
    ids, lin, rank, _ = cases.toy_table()
    os.makedirs(os.path.join(HERE, "merge_cases_in"), exist_ok=True)
    for name, data in cases.generated_files(ids, rank).items():
        with open(os.path.join(HERE, "merge_cases_in", name + ".txt"), "wb") as f:
            f.write(data)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, (files, args) in CASES.items():
            res = os.path.join(tmp, name + ".txt")
            r = subprocess.run([REF, "merge"] + files + ["-taxonomy", TAX] + args + ["-out", res], cwd=HERE, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(f"FAILED: {name}\n{r.stdout}\n{r.stderr}")
            out[name] = {"files": files, "args": args, "lines": open(res).read().split("\n")}
    with gzip.open(os.path.join(HERE, "merge_cases_expected.json.gz"), "wt") as f:
        json.dump(out, f)
    print({k: len(v["lines"]) for k, v in out.items()})


if __name__ == "__main__":
    main()
