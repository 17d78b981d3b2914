"""Writes the index cases of tests/test_inflate_witness_cpu.py as files into a directory, for tools/bgzf_rules_check.cpp:
    python tools/bgzf_rules_cases.py <dir>"""
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import inflate_cases as cases   # noqa: E402
import inflate_ref as ref       # noqa: E402


def main(out):
    os.makedirs(out, exist_ok=True)
    good = cases.good_cases()
    m, plain = good["one_byte"]
    raw = ref.payload_of(m)
    three = good["short_text"][0] + m + cases.EOF_BLOCK
    files = {"all_good": b"".join(good[n][0] for n in sorted(good)), "three": three, "empty": b"", "eof_only": cases.EOF_BLOCK,
             "flg_0c": m[:3] + b"\x0c" + m[4:], "no_bc": m[:12] + b"XX" + m[14:], "bc_twice": cases.member(raw, plain, extra=b"BC\x02\x00\x00\x00"),
             "bc_behind": good["bc_behind_another_subfield"][0], "cut_short": three[:-1], "trailing": three + b"\x00", "trailing_header": three + three[:11],
             "isize_65537": m[:-4] + struct.pack("<I", 65537), "xlen_huge": m[:10] + b"\xff\xff" + m[12:], "bsize_small": m[:16] + b"\x05\x00" + m[18:]}
    untiled = bytearray(cases.member(raw, plain, extra=b"XY\x03\x00abc")); untiled[14] = 4
    files["untiled"] = bytes(untiled)
    with open(os.path.join(ROOT, "tests", "golden", "cli_reads.fa.gz"), "rb") as f:
        files["plain_gzip"] = f.read()
    for name, data in files.items():
        with open(os.path.join(out, name), "wb") as f:
            f.write(data)
    print(" ".join(os.path.join(out, n) for n in sorted(files)))


if __name__ == "__main__":
    main(sys.argv[1])
