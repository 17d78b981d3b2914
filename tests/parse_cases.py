"""Generated FASTA / FASTQ inputs for the parse tests (test_gpu_parse, test_parse_witness_cpu): files built around a tile of T bytes, every
one also with '\\r\\n' line ends, and the regular golden read files.  all_cases(T) -> {name: bytes}; every one is regular under the rule."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCAN_TRIP = 256                              # tile sums parse_scan_kernel takes per trip
REGULAR = ["cli_reads.fa", "cli_pairs.fq", "cli_truth.fa", "cli_p1.fa", "cli_fmt.fa"]
IRREGULAR = ["cli_irregular.fa", "cli_irregular.fq"]


def golden_bytes(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


TAIL_ZONES = ("one_tile", "tile_border")


def dna(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


def fasta_record(name, seq, width=0, comment=b""):
    body = seq if not width else b"\n".join(seq[k:k + width] for k in range(0, len(seq), width))
    return b">" + name + comment + b"\n" + body + (b"\n" if body else b"")


def fastq_record(name, seq, qual=None, comment=b""):
    return b"@" + name + comment + b"\n" + seq + b"\n+\n" + (qual if qual is not None else b"I" * len(seq)) + b"\n"


def pad_to(prefix_len, target, rng, fastq, nl=1):
    """records that take exactly target - prefix_len bytes (with line ends of nl bytes)"""
    room = target - prefix_len
    out = []
    while room > 0:
        fixed = (3 + 4 * nl) if fastq else (2 + 2 * nl)          # the markers ('+' included), a one-byte name and the line ends
        take = room if room < 2 * (fixed + 40) + 80 else fixed + 40
        k = take - fixed
        assert k >= 2, (room, take)
        if fastq:
            s = dna(rng, k // 2)
            out.append(b"@" + b"n" * (1 + k - 2 * (k // 2)) + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n")
        else:
            out.append(b">n\n" + dna(rng, k) + b"\n")
        if nl == 2:
            out[-1] = out[-1].replace(b"\n", b"\r\n")
        assert len(out[-1]) == take, (len(out[-1]), take)
        room -= take
    return b"".join(out)


def border_cases(T):
    """name -> bytes, LF line ends; the CRLF twins are made by the caller"""
    rng = np.random.default_rng(5)
    cases = {}
    for fq in (False, True):
        rec = fastq_record if fq else fasta_record
        k = "fq" if fq else "fa"
        a = pad_to(0, T, rng, fq)
        cases[f"marker_at_T_{k}"] = a + rec(b"atT", dna(rng, 70)) + rec(b"after desc", dna(rng, 33))
        assert cases[f"marker_at_T_{k}"][T:T + 1] in (b">", b"@") and cases[f"marker_at_T_{k}"][T - 1:T] == b"\n"
        # a header across the border, and the name's blank exactly at T
        head = pad_to(0, T - 10, rng, fq)
        cases[f"header_across_{k}"] = head + rec(b"x" * 30, dna(rng, 50), comment=b" tail of the header") + rec(b"z", dna(rng, 9))
        cases[f"blank_at_T_{k}"] = head + rec(b"y" * 9, dna(rng, 50), comment=b" blank is at T") + rec(b"z", dna(rng, 9))
        assert cases[f"blank_at_T_{k}"][T:T + 1] == b" "
        cases[f"single_{k}"] = rec(b"only one", dna(rng, 101))
        cases[f"no_final_newline_{k}"] = (rec(b"a", dna(rng, 40)) + rec(b"b 2", dna(rng, 41)))[:-1]
        cases[f"many_tiles_{k}"] = b"".join(rec(b"r%d c" % i, dna(rng, 100 + i % 50)) for i in range((SCAN_TRIP + 3) * T // (240 if fq else 120)))
        assert len(cases[f"many_tiles_{k}"]) > (SCAN_TRIP + 1) * T
    long_seq = dna(rng, 5 * T // 2)
    cases["long_record_fa"] = fasta_record(b"before", dna(rng, 77), 60) + fasta_record(b"long one", long_seq, 60) + fasta_record(b"behind", dna(rng, 61), 60)
    cases["long_record_fq"] = fastq_record(b"before", dna(rng, 77)) + fastq_record(b"long one", long_seq) + fastq_record(b"behind", dna(rng, 61))
    cases["empty_sequence_fa"] = fasta_record(b"a", dna(rng, 20)) + b">empty here\n" + fasta_record(b"c", dna(rng, 21)) + b">last is empty\n"
    cases["blank_lines_fa"] = b">a\nACGT\n\nGGTT\n\n>b\n\nAC\n"
    cases["markers_inside_fa"] = b">a >b @c\nAC>GT\n@CGT\nAC@+\n>b\nA+C\n"
    cases["markers_inside_fq"] = fastq_record(b"a @x >y", b"AC@G>T+A", b"@>+@II+I") + fastq_record(b"b", b"ACGT", b"@III") + fastq_record(b"c", b"GG", b"+@")
    # '\n' at T - 1 with a sequence line behind it (no marker at T)
    cases["newline_before_T_fa"] = b">n\n" + dna(rng, T - 4) + b"\n" + dna(rng, 30) + b"\n>z\nAC\n"
    assert cases["newline_before_T_fa"][T - 1:T] == b"\n"
    return cases


def crlf(data):
    return data.replace(b"\n", b"\r\n")


def crlf_at_border(T, fq):
    """'\\r' at T - 1 with '\\n' at T: the end of a sequence line"""
    rng = np.random.default_rng(6)
    if fq:
        s = dna(rng, T - 5)
        d = b"@n\r\n" + s + b"\r\n+\r\n" + b"I" * len(s) + b"\r\n" + crlf(fastq_record(b"z", b"ACGT"))
    else:
        d = b">n\r\n" + dna(rng, T - 5) + b"\r\n" + dna(rng, 30) + b"\r\n>z\r\nAC\r\n"
    assert d[T - 1:T + 1] == b"\r\n"
    return d


def all_cases(T):
    cases = border_cases(T)
    out = dict(cases)
    for k, v in cases.items():
        out[k + "_crlf"] = crlf(v)
    out["cr_before_T_fa"] = crlf_at_border(T, False)
    out["cr_before_T_fq"] = crlf_at_border(T, True)
    # the marker at T behind '\r\n'
    rng = np.random.default_rng(7)
    for fq in (False, True):
        a = pad_to(0, T, rng, fq, nl=2)
        out[f"marker_at_T_{'fq' if fq else 'fa'}_crlf2"] = a + crlf((fastq_record if fq else fasta_record)(b"atT", dna(rng, 70)))
    for name in REGULAR:
        out[name] = golden_bytes(name)
    out.update(tail_sweep(T))
    return out


def tail_sweep(T):
    """a range that ends inside a thread's 16 bytes: one FASTA file cut to every length L .. L + 15, inside one tile and with
    T - 8 <= L < T + 8 around the tile border, its last line whole and without its final '\\n'"""
    rng = np.random.default_rng(8)
    last = fasta_record(b"last one", dna(rng, 21))
    out = {}
    for zone, L in zip(TAIL_ZONES, (208, T - 8)):
        for i in range(16):
            out[f"tail_{zone}_{i:02d}_fa"] = pad_to(0, L + i - len(last), rng, False) + last
            out[f"tail_{zone}_{i:02d}_cut_fa"] = (pad_to(0, L + i + 1 - len(last), rng, False) + last)[:-1]
            assert len(out[f"tail_{zone}_{i:02d}_fa"]) == len(out[f"tail_{zone}_{i:02d}_cut_fa"]) == L + i
    return out


CASE_NAMES = sorted(["marker_at_T", "header_across", "blank_at_T", "single", "no_final_newline", "many_tiles", "long_record", "markers_inside"][i] + s
                    for i in range(8) for s in ("_fa", "_fq", "_fa_crlf", "_fq_crlf")) + \
    ["empty_sequence_fa", "empty_sequence_fa_crlf", "blank_lines_fa", "blank_lines_fa_crlf", "newline_before_T_fa", "newline_before_T_fa_crlf",
     "cr_before_T_fa", "cr_before_T_fq", "marker_at_T_fa_crlf2", "marker_at_T_fq_crlf2"] + REGULAR + \
    [f"tail_{zone}_{i:02d}{cut}_fa" for zone in TAIL_ZONES for i in range(16) for cut in ("", "_cut")]
