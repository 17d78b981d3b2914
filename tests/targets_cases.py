"""Generated inputs for the target parse tests (test_gpu_targets, test_targets_witness_cpu, test_cpp_parse_targets): lists of FASTA files
built around a tile of T bytes, every one also with '\\r\\n' line ends, the golden genome files, irregular ranges and bad file tables.
regular_cases(T) -> {name: [file bytes]}; irregular_cases(T) -> {name: ([file bytes], file of the offence, offset of the offence in that
file)}; bad_tables() -> {name: (data, file_off, first bad row)}."""
import os

import numpy as np

from parse_cases import GOLDEN, SCAN_TRIP, crlf, dna, fasta_record, pad_to

GENOMES = os.path.join(GOLDEN, "build_in", "genomes")
GENOME_FILES = ["GCF_000001111.1_ASM111v1_genomic.fna", "mixed.fa", os.path.join("sub", "GCF_000002222.2_other.fa")]


def genome_bytes(name):
    with open(os.path.join(GENOMES, name), "rb") as f:
        return f.read()


def lf_cases(T):
    rng = np.random.default_rng(11)
    cases = {}
    tail = [fasta_record(b"second file", dna(rng, 90), 60) + fasta_record(b"its second", dna(rng, 31), 60)]
    # a file start at T - 1, T, T + 1
    for d in (-1, 0, 1):
        cases[f"file_start_at_T{d:+d}"] = [pad_to(0, T + d, rng, False)] + tail
    # a file without a final '\n' that ends at T - 1 and at T, another file behind it
    for d in (-1, 0):
        first = pad_to(0, T + d + 1, rng, False)[:-1]
        assert len(first) == T + d and not first.endswith(b"\n")
        cases[f"no_final_newline_end_at_T{d:+d}"] = [first] + tail
    # twenty files of ">" or ">\n" in a row: several file starts inside one thread's 16 bytes
    cases["tiny_files"] = [fasta_record(b"front", dna(rng, 13))] + [b">" if k % 3 else b">\n" for k in range(20)] + [b">x\nAC"]
    cases["tiny_files_only"] = [b">"] * 20
    # a record whose sequence spans three tiles on lines of 60
    cases["long_record"] = [fasta_record(b"before", dna(rng, 77), 60), fasta_record(b"long one", dna(rng, 5 * T // 2), 60) + fasta_record(b"behind", dna(rng, 61), 60)]
    cases["blank_lines"] = [b">a\nACGT\n\nGGTT\n\n>b\n\nAC\n", b">c\n\n\nA\n\n"]
    # empty records first, in the middle and last in a file
    cases["empty_records"] = [b">first is empty\n" + fasta_record(b"a", dna(rng, 20)) + b">empty here\n" + fasta_record(b"c", dna(rng, 21)) + b">last is empty\n",
                              b">e\n>f\nACG\n>g", b">h\nT\n"]
    # a header across a tile border
    head = pad_to(0, T - 10, rng, False)
    cases["header_across"] = [head + fasta_record(b"x" * 30, dna(rng, 50), comment=b" tail of the header"), fasta_record(b"z", dna(rng, 9))]
    cases["header_across_file_end"] = [head + b">" + b"h" * 30, fasta_record(b"z", dna(rng, 9))]
    # one range of 256 tiles and a few bytes: more than one trip of the scan over the tile sums
    files, total, k = [], 0, 0
    while total <= SCAN_TRIP * T + 40:
        f = b"".join(fasta_record(b"r%d.%d c" % (k, i), dna(rng, 900 + 37 * i), 70) for i in range(1 + k % 3))
        files.append(f); total += len(f); k += 1
    cases["many_tiles"] = files
    cases["single_file"] = [fasta_record(b"only one", dna(rng, 101))]
    # seq needs MORE bytes than the range holds: an empty header, no final '\n', len % 4 == 1 at a file's end -- one byte per such file
    cases["tight_tail_1"] = [b">\nA"]
    cases["tight_tail_5"] = [b">\nACGTA"]
    cases["tight_tails_in_a_row"] = [b">\nA", b">\nACGTA", b">\nG"] * 7 + [b">\nACGTACGTA"]
    return cases


def regular_cases(T):
    out = {}
    for name, files in lf_cases(T).items():
        out[name] = files
        out[name + "_crlf"] = [crlf(f) for f in files]
    # '\r' as the last byte of a file without '\n': trimmed, not refused
    out["cr_at_file_end"] = [b">a\r\nACGT\r", b">b\r", b">c\r\nAC\r\n"]
    genomes = [genome_bytes(n) for n in GENOME_FILES]
    out["golden_genomes"] = genomes
    out["golden_genomes_crlf"] = [crlf(g) for g in genomes]
    return out


REGULAR_NAMES = sorted([n + s for n in ["file_start_at_T-1", "file_start_at_T+0", "file_start_at_T+1", "no_final_newline_end_at_T-1", "no_final_newline_end_at_T+0",
                                         "tiny_files", "tiny_files_only", "long_record", "blank_lines", "empty_records", "header_across", "header_across_file_end",
                                         "many_tiles", "single_file", "golden_genomes", "tight_tail_1", "tight_tail_5", "tight_tails_in_a_row"] for s in ("", "_crlf")] + ["cr_at_file_end"])


def irregular_cases(T):
    rng = np.random.default_rng(12)
    good = fasta_record(b"good", dna(rng, 2 * T + 5), 60)
    lf = {
        "fastq_file": ([good, b"@r\nACGT\n+\nIIII\n", good], 1, 0),
        "sequence_first": ([good, b"ACGT\n>late\nAC\n"], 1, 0),
        "plus_line": ([good, b">a\nAC\n+\nGG\n"], 1, 6),
        "lone_cr": ([b">a\nAC\rGT\n", good], 0, 5),
        "two_offenders": ([good, b">a\n+\n", good, b"@q\n"], 1, 3),
        "empty_line_first": ([good, b"\n>a\nAC\n"], 1, 0),
    }
    out = dict(lf)
    for name, (files, f, at) in lf.items():
        if name == "lone_cr":
            continue
        twin = [crlf(x) for x in files]
        out[name + "_crlf"] = (twin, f, at + files[f][:at].count(b"\n"))
    out["cr_before_file_end_byte"] = ([b">a\nAC\rG", good], 0, 5)
    return out


IRREGULAR_NAMES = sorted([n + s for n in ["fastq_file", "sequence_first", "plus_line", "two_offenders", "empty_line_first"] for s in ("", "_crlf")] + ["lone_cr", "cr_before_file_end_byte"])


def bad_tables():
    data = b">a\nACGT\n>b\nGG\n>c\nT\n"
    n = len(data)
    return {
        "first_row_not_0": (data, np.array([1, 8, n], dtype=np.uint64), 0),
        "equal_rows": (data, np.array([0, 8, 8, n], dtype=np.uint64), 2),
        "descending_rows": (data, np.array([0, 14, 8, n], dtype=np.uint64), 2),
        "last_row_not_nbytes": (data, np.array([0, 8, n - 1], dtype=np.uint64), 2),
        "last_row_beyond": (data, np.array([0, 8, n + 5], dtype=np.uint64), 2),
    }


BAD_TABLE_NAMES = sorted(["first_row_not_0", "equal_rows", "descending_rows", "last_row_not_nbytes", "last_row_beyond"])
