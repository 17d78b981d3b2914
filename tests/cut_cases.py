"""Inputs for the cut tests (test_cut_witness_cpu, test_gpu_cut): the generated files of parse_cases.all_cases(T), the golden read files
(the irregular ones too), and ranges whose END is the point -- each with '\\n' and with '\\r\\n' line ends.
all_cases(T) -> {name: (bytes, pairs)}; open_cases() -> {name: (bytes, pairs)} are meant for MC_CUT_OPEN (and are cut closed as well)."""
import numpy as np

import parse_cases
from parse_cases import crlf, dna, fasta_record, fastq_record


def open_cases():
    rng = np.random.default_rng(11)
    fq = [fastq_record(b"q%d x" % i, dna(rng, 30 + i)) for i in range(7)]
    fa = [fasta_record(b"a%d y" % i, dna(rng, 50 + 3 * i), 20) for i in range(7)]
    cases = {}
    tail = fastq_record(b"tail", dna(rng, 25))
    lines = tail.split(b"\n")[:-1]
    for k in (1, 2, 3):
        cases[f"fq_tail_{k}_lines"] = (b"".join(fq[:4]) + b"\n".join(lines[:k]) + b"\n", False)
        cases[f"fq_tail_{k}_lines_cut"] = (b"".join(fq[:4]) + b"\n".join(lines[:k]), False)              # the k-th line itself is cut short
    cases["fq_tail_4_lines_no_newline"] = (b"".join(fq[:4]) + tail[:-1], False)
    cases["fq_ends_whole"] = (b"".join(fq[:5]), False)
    cases["fq_first_group_cut"] = (fq[0][:-5], False)
    cases["fa_one_record"] = (fa[0], False)
    cases["fa_one_record_no_newline"] = (fa[0][:-1], False)
    cases["fa_several"] = (b"".join(fa[:5]), False)
    cases["fa_last_header_cut"] = (b"".join(fa[:4]) + b">cut he", False)
    cases["fa_marker_is_last_byte"] = (b"".join(fa[:4]) + b">", False)
    cases["fq_pairs_odd_whole"] = (b"".join(fq[:5]) + tail[:20], True)
    cases["fq_pairs_even_whole"] = (b"".join(fq[:6]) + tail[:20], True)
    cases["fq_pairs_ends_odd"] = (b"".join(fq[:5]), True)
    cases["fa_pairs_odd_whole"] = (b"".join(fa[:6]), True)                                             # open: 5 whole -> 4
    cases["fa_pairs_even_whole"] = (b"".join(fa[:5]), True)
    cases["fa_pairs_two"] = (b"".join(fa[:2]), True)
    # an offence just in front of consumed and one just behind it
    bad_fq = b"@bad\n+ACGT\n+\nIIII\n"                                                                # the sequence line starts with '+'
    cases["fq_offence_in_front"] = (b"".join(fq[:3]) + bad_fq + tail[:30], False)
    cases["fq_offence_behind"] = (b"".join(fq[:3]) + bad_fq[:-3], False)
    cases["fa_offence_in_front"] = (b"".join(fa[:2]) + b">bad\nACGT\n+\nAC\n" + fa[3], False)
    cases["fa_offence_behind"] = (b"".join(fa[:3]) + b">open\nACGT\n+\nAC\n", False)                   # a '+' line start inside the open record
    cases["fa_plus_in_open_header_line"] = (b"".join(fa[:3]) + b">open\n+", False)
    out = dict(cases)
    for k, (d, p) in cases.items():
        out[k + "_crlf"] = (crlf(d), p)
    return out


def all_cases(T):
    out = {k: (v, False) for k, v in parse_cases.all_cases(T).items()}
    for name in parse_cases.IRREGULAR:
        out[name] = (parse_cases.golden_bytes(name), False)
    out["cli_pairs.fq_pairs"] = (parse_cases.golden_bytes("cli_pairs.fq"), True)
    out["cli_fmt.fa_pairs"] = (parse_cases.golden_bytes("cli_fmt.fa"), True)
    out.update(open_cases())
    return out
