"""The mates model (parse_mates_ref) against the single-range model it restates: for accepted ranges its outputs equal
parse_ref.pack(interleaved, pairs=True) on a file in which the two ranges' records alternate; unequal counts and an offence in either
range give the verdicts and status words of include/metacache_amd.h.  No GPU: this keeps the model honest, the device tests use it."""
import numpy as np
import pytest

import parse_mates_cases
import parse_mates_ref as mref
import parse_ref
from parse_cases import dna, fasta_record, fastq_record, golden_bytes

T = 4096
CASES = None


def cases():
    global CASES
    if CASES is None:
        CASES = parse_mates_cases.all_cases(T)
    return CASES


def test_case_list_is_complete():
    assert sorted(cases()) == parse_mates_cases.CASE_NAMES


@pytest.mark.parametrize("name", parse_mates_cases.CASE_NAMES)
def test_model_equals_the_pairs_of_the_interleaved_file(name):
    d1, d2 = cases()[name]
    got = mref.mates(d1, d2, insert_max=180, stride=113)
    both = mref.interleave(d1, d2)
    want = parse_ref.pack(both, parse_ref.parse(both), pairs=True, insert_max=180, stride=113)
    assert [int(x) for x in got["status"][:8]] == [int(x) for x in want["status"]]
    assert int(got["status"][8]) == int(got["status"][9]) == int(want["status"][1])
    for key in ("qinfo", "name_off", "max_win"):
        assert np.array_equal(got[key], want[key]), key
    assert got["seq"] == want["seq"] and got["names"] == want["names"]
    assert np.array_equal(got["hdr"][:, 1], want["hdr"][:, 1])
    for q in range(len(got["qinfo"])):                           # hdr: places in the range the mate came from
        for f, d in ((0, d1), (1, d2)):
            off, length = (int(x) for x in got["hdr"][2 * q + f])
            w = int(want["hdr"][2 * q + f, 0])
            assert d[off:off + length] == both[w:w + length] and d[off - 1:off] in (b">", b"@")


def test_golden_pair_files_are_the_cli_pairs():
    d1, d2 = golden_bytes("cli_p1.fa"), golden_bytes("cli_p2.fa")
    got = mref.mates(d1, d2)
    r1, r2 = parse_ref.parse(d1).records, parse_ref.parse(d2).records
    assert int(got["status"][4]) == mref.OK and len(r1) == len(r2) == int(got["status"][1]) > 0
    for q, (a, b) in enumerate(zip(r1, r2)):
        o1, l1, o2, l2 = (int(x) for x in got["qinfo"][q])
        assert got["seq"][o1:o1 + l1] == a[2] and got["seq"][o2:o2 + l2] == b[2]


def test_unequal_counts():
    rng = np.random.default_rng(3)
    recs = [fasta_record(b"r%d" % i, dna(rng, 30 + i)) for i in range(6)]
    for n1, n2 in ((6, 5), (5, 6)):
        got = mref.mates(b"".join(recs[:n1]), b"".join(recs[:n2]))
        st = [int(x) for x in got["status"]]
        assert (st[0], st[4], st[7], st[8], st[9]) == (n1 + n2, mref.UNEQUAL, 0, n1, n2) and set(got) == {"status"}


def test_offence_in_either_range():
    rng = np.random.default_rng(4)
    good = b"".join(fastq_record(b"r%d" % i, dna(rng, 30)) for i in range(4))
    bad = good + b"stray\n" + good
    bad2 = b"@a\nACGT\nno plus\nIIII\n" + good
    assert parse_ref.parse(bad2).offence == 8
    for d1, d2, rng_no, off in ((bad, good, 0, len(good)), (good, bad, 1, len(good)), (bad, bad2, 0, len(good)), (bad2, bad, 0, parse_ref.parse(bad2).offence)):
        st = [int(x) for x in mref.mates(d1, d2)["status"]]
        assert (st[4], st[5], st[7]) == (mref.IRREGULAR, off, rng_no)


def test_overflow_reports_the_needs():
    d1, d2 = cases()["lengths_mod_4"]
    full = mref.mates(d1, d2)
    need = [int(x) for x in full["status"]]
    assert need[0] == 32 and need[1] == 16 and need[6] == 11 + 7
    for kw in (dict(max_records=31), dict(seq_capacity=need[2] - 1), dict(names_capacity=need[3] - 1)):
        got = mref.mates(d1, d2, **kw)
        st = [int(x) for x in got["status"]]
        assert st[4] == mref.OVERFLOW and st[:4] == need[:4] and st[8:] == [16, 16] and set(got) == {"status"}
        assert st[6] == (0 if "max_records" in kw else need[6])
