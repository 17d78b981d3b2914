#!/usr/bin/env python3
"""Golden vector for the ranking pass: what the REFERENCE's `build -taxpostmap` made of the witness records and table of
tests/taxmap_cases.py (needs oracle/_ref/metacache_u32 = the reference compiled by `make -C oracle ref`).  Writes data only:

  taxmap_expected.json      {"parents": {target name: parent taxid}} as read back from the .meta file the reference wrote

Usage:  python tests/golden/make_golden_taxmap.py
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import taxmap_cases as cases  # noqa: E402

REF32 = os.path.join(ROOT, "oracle", "_ref", "metacache_u32")


def main():
    if not os.path.exists(REF32):
        sys.exit("oracle/_ref is missing: run `make -C oracle ref` first")
    with tempfile.TemporaryDirectory() as tmp:
        parents = cases.run_witness(REF32, tmp)
    with open(os.path.join(HERE, "taxmap_expected.json"), "w") as f:
        json.dump({"parents": {k.decode(): v for k, v in sorted(parents.items())}}, f, indent=1)
        f.write("\n")
    print("wrote taxmap_expected.json:", parents)


if __name__ == "__main__":
    main()
