"""Pairs of ranges for mc_parse_mates, built around the tile T = api.parse_tile() and around what the per-record passes take: a block
of mates_sums_kernel / mates_place_kernel 256 queries, one trip of mates_scan_kernel 256 such blocks.  Shared by the model's witness
(CPU) and the device tests; all_cases(T) -> name -> (bytes of range 1, bytes of range 2), built once."""
import numpy as np

import parse_ref
from parse_cases import crlf, dna, fasta_record, fastq_record, golden_bytes, pad_to

QUERY_BLOCK = 256                            # queries a block of the per-record passes takes
QUERY_TRIP = 256 * QUERY_BLOCK               # queries one trip of the per-record scan takes
COUNTS = [QUERY_BLOCK - 1, QUERY_BLOCK, QUERY_BLOCK + 1, QUERY_TRIP - 1, QUERY_TRIP, QUERY_TRIP + 1]


def count_records(data):
    p = parse_ref.parse(data)
    assert p.verdict == parse_ref.OK
    return len(p.records)


def short_records(n, rng, fq=False, first=0):
    """n records of 1 .. 12 bases: a whole file of them stays small"""
    rec = fastq_record if fq else fasta_record
    return b"".join(rec(b"m%d" % (first + i), dna(rng, 1 + int(rng.integers(0, 12)))) for i in range(n))


def tiny_records(n):
    """n records of 1 .. 5 bases, a few bytes each (the counts around the per-record scan's trip)"""
    return b"".join(b">%x\n%s\n" % (i, b"ACGTA"[:1 + i % 5]) for i in range(n))


def all_cases(T):
    rng = np.random.default_rng(17)
    c = {}
    for fq in (False, True):
        k = "fq" if fq else "fa"
        rec = fastq_record if fq else fasta_record
        a = pad_to(0, T, rng, fq) + rec(b"atT", dna(rng, 70)) + rec(b"after desc", dna(rng, 33))
        assert a[T - 1:T] == b"\n" and a[T:T + 1] in b">@"
        other = short_records(count_records(a), rng, fq)
        assert len(other) < T
        c[f"borders_in_1_{k}"] = (a, other)
        c[f"borders_in_2_{k}"] = (other, a)
        h = pad_to(0, T - 10, rng, fq) + rec(b"x" * 30, dna(rng, 50), comment=b" tail of the header") + rec(b"z", dna(rng, 9))
        o = short_records(count_records(h), rng, not fq)
        assert len(o) < T
        c[f"header_across_in_1_{k}"] = (h, o)
        c[f"header_across_in_2_{k}"] = (o, h)
    # one tile beside more than 256 tiles
    n = 300
    one = short_records(n, rng)
    many = b"".join(fasta_record(b"long%d of many" % i, dna(rng, 3600 + i % 7), 60) for i in range(n))
    assert len(one) <= T and len(many) > 257 * T
    c["one_tile_beside_many"] = (one, many)
    c["many_beside_one_tile"] = (many, one)
    # 2.5 T opposite an empty sequence
    long_one = fasta_record(b"before", dna(rng, 77), 60) + fasta_record(b"long one", dna(rng, 5 * T // 2), 60) + fasta_record(b"behind", dna(rng, 61), 60)
    empty = fasta_record(b"a", dna(rng, 20)) + b">empty here\n" + fasta_record(b"c", dna(rng, 21))
    c["long_opposite_empty"] = (long_one, empty)
    c["empty_opposite_long"] = (empty, long_one)
    long_fq = fastq_record(b"before", dna(rng, 77)) + fastq_record(b"long one", dna(rng, 5 * T // 2)) + fastq_record(b"behind", dna(rng, 61))
    c["long_fq_opposite_empty"] = (long_fq, empty)
    # all 16 combinations of len1 % 4, len2 % 4
    c["lengths_mod_4"] = (b"".join(fasta_record(b"p%d/1 c" % i, dna(rng, 8 + i // 4)) for i in range(16)),
                          b"".join(fastq_record(b"p%d/2" % i, dna(rng, 4 + i % 4)) for i in range(16)))
    fa = b"".join(fasta_record(b"q%d first mate" % i, dna(rng, 90 + 7 * i), 60) for i in range(40))
    fq = b"".join(fastq_record(b"q%d" % i, dna(rng, 151 - i), comment=b" second") for i in range(40))
    c["fasta_beside_fastq"] = (fa, fq)
    c["fastq_beside_fasta"] = (fq, fa)
    c["crlf_in_1"] = (crlf(fa), fq)
    c["crlf_in_2"] = (fa, crlf(fq))
    c["no_final_newline_in_1"] = (fa[:-1], fq)
    c["no_final_newline_in_2"] = (fa, fq[:-1])
    c["single_query"] = (fasta_record(b"only one", dna(rng, 101)), fastq_record(b"its mate", dna(rng, 99)))
    c["golden_p1_p2"] = (golden_bytes("cli_p1.fa"), golden_bytes("cli_p2.fa"))
    for n in COUNTS:
        c[f"count_{n}"] = (tiny_records(n), tiny_records(n + 3)[len(tiny_records(3)):])
        assert count_records(c[f"count_{n}"][1]) == n if n < 1000 else True
    return c


CASE_NAMES = sorted([f"{a}_{k}" for a in ("borders_in_1", "borders_in_2", "header_across_in_1", "header_across_in_2") for k in ("fa", "fq")] +
                    ["one_tile_beside_many", "many_beside_one_tile", "long_opposite_empty", "empty_opposite_long", "long_fq_opposite_empty", "lengths_mod_4",
                     "fasta_beside_fastq", "fastq_beside_fasta", "crlf_in_1", "crlf_in_2", "no_final_newline_in_1", "no_final_newline_in_2", "single_query",
                     "golden_p1_p2"] + [f"count_{n}" for n in COUNTS])
FASTA_ONLY = ["borders_in_1_fa", "one_tile_beside_many", "long_opposite_empty", "golden_p1_p2", "count_257"]   # both ranges FASTA
