"""Writes the rows of tests/gzip_cases.py as files into a directory, for tools/gzip_rules_check.cpp:
    python tools/gzip_rules_cases.py <dir>"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gzip_cases as cases   # noqa: E402


def main(out):
    os.makedirs(out, exist_ok=True)
    files = {"good_" + n: r[0] for n, r in cases.good_cases().items()}
    files.update({"bad_" + n: r[0] for n, r in cases.bad_cases().items()})
    files["empty"] = b""
    with open(os.path.join(ROOT, "tests", "golden", "build_in", "genomes", "more.fa.gz"), "rb") as f:
        files["golden_more_fa_gz"] = f.read()
    for name, data in files.items():
        with open(os.path.join(out, name), "wb") as f:
            f.write(data)
    print(" ".join(os.path.join(out, n) for n in sorted(files)))


if __name__ == "__main__":
    main(sys.argv[1])
