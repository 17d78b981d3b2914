"""CPU: the plain model of `query -align` (tests/align_ref.py) reproduces EVERY alignment the reference program printed
(tests/golden/align_expected.json.gz, made by tests/golden/make_golden_align.py) when it reads the record the reference reads: the one
BEFORE the target's own.  The first alignment line names file, record number and window range, so the cut is known; the read and its
mate come from the reads file, the record from build_in.  That pins the model -- recurrence, tie rules, end cell, orientation choice,
cut, the three lines -- to the reference; tests/test_gpu_align.py and tests/test_cli_align_gpu.py then use the same model with mcq's
record rule."""
import gzip
import json
import os

import pytest

import align_ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
GENOME_FILES = ["build_in/genomes/GCF_000001111.1_ASM111v1_genomic.fna", "build_in/genomes/mixed.fa", "build_in/genomes/more.fa.gz",
                "build_in/genomes/sub/GCF_000002222.2_other.fa"]


def _cases():
    p = os.path.join(GOLD, "align_expected.json.gz")
    if not os.path.exists(p):
        return {}
    with gzip.open(p, "rt") as f:
        return json.load(f)["cases"]


CASES = _cases()
NAMES = ["align", "align_tophits", "align_mapped_only", "align_species", "align_maxcand", "align_pairs", "align_long", "align_cov", "align_w64",
         "align_elsewhere"]
WITHOUT_LINES = {"align_species", "align_elsewhere"}


def test_the_goldens_hold_every_case():
    assert sorted(CASES) == sorted(NAMES)


@pytest.mark.parametrize("case", NAMES)
def test_model_reproduces_every_alignment_of_the_reference(case):
    c = CASES[case]
    comment, sep = align_ref.option(c["args"], "-comment", "# "), align_ref.option(c["args"], "-separator", "\t|\t")
    winlen, stride = align_ref.SKETCHING[c["db"]]
    reads = align_ref.queries(os.path.join(GOLD, c["reads"]), "-pairseq" in c["args"])
    records = align_ref.Records(GOLD)
    cols = align_ref.columns(c["lines"], comment, sep)
    name_col = cols.index("query_header")
    n = 0
    for i, line, aln in align_ref.parse_output(c["lines"], comment):
        if aln is None:
            continue
        n += 1
        read, mate = reads[line.split(sep)[name_col]]
        if "-cov-percentile" in c["args"]:      # the reference keeps no sequences for the pass after the coverage filter: it aligns an empty query
            read, mate = b"", None
        score, filename, index, beg, end = align_ref.parse_head(aln[0], comment, stride)
        exp = align_ref.alignment_lines(records, "reference", comment, filename, index, beg, end, winlen, stride, read, mate)
        assert exp == aln, (case, i, line[:80], exp and exp[0], aln[0])
    assert (n == 0) == (case in WITHOUT_LINES), (case, n)


@pytest.mark.parametrize("case", [k for k in NAMES if any(a in ("-tophits", "-locations") for a in CASES.get(k, {}).get("args", []))])
def test_reference_drops_targets_that_open_their_file(case):
    """a first candidate that is the first record of its source file: the reference skips past the end of the file and prints nothing"""
    c = CASES[case]
    comment, sep = align_ref.option(c["args"], "-comment", "# "), align_ref.option(c["args"], "-separator", "\t|\t")
    top = align_ref.columns(c["lines"], comment, sep).index("top_hits")
    first = align_ref.first_record_names(GOLD, GENOME_FILES)
    seen = 0
    for i, line, aln in align_ref.parse_output(c["lines"], comment):
        cand = line.split(sep)[top].split(",")[0]
        if cand and cand.rsplit(":", 1)[0] in first:
            seen += 1
            assert aln is None, (case, i, line[:120])
    assert seen > 0, case
