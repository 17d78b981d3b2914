"""`mcq query` with MCQ_FORMAT_DEVICE=1: a worker hands every batch's candidate rows to mc_classify_candidates and mc_format_mappings and
takes its tallies from the assignments; the host loop (classify + MappingWriter) is not run for those batches.

  * golden cases of tests/golden/cli_expected.json.gz (the reference's own output) that between them use every column, every option
    that shapes a taxon's text, pairs, two files, -abundances, -ground-truth, -precision and -hits-per-ref must come out line for line,
    and MCQ_PROFILE must say that every read went through the library and no batch stayed on the host;
  * the 144 option combinations of format_matrix, typed into one interactive session (the tables are made again for every job);
  * -allhits, -cov-percentile and -maxcand 0 keep the host loop: the goldens still come out, and MCQ_PROFILE says so and why;
  * without the switch stderr holds no word about it."""
import gzip
import json
import os
import re
import subprocess

import pytest

from metacache_amd import build

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")

DEVICE_CASES = ["default", "genus_family_idsonly", "separate_cols", "mapped_only_vote", "hitdiff_percent", "separator", "pairseq_insert", "two_files",
                "locations", "locations_pairs", "abundances_species", "ground_truth", "precision", "hits_per_ref_lineage", "comment_token"]
HOST_CASES = {"everything_species": "-allhits", "cov_percentile": "-cov-percentile", "maxcand_unlimited": "-maxcand 0"}


def cli_case(name):
    with gzip.open(os.path.join(GOLD, "cli_expected.json.gz"), "rt") as f:
        return json.load(f)[name]


def volatile(line):
    return re.match(r"^(# |%%)(time:    |speed:   |Using \d+ threads$)", line) is not None


def same_lines(got, exp, tag, lists_unordered=False):
    """line for line; lists_unordered: the lines of -hits-per-ref's table, which the reference prints in the iteration order of an
    unordered_map (tests/test_cli_gpu.py compares them the same way), are sorted on both sides -- they stay where the table is"""
    assert len(got) == len(exp), (tag, len(got), len(exp))
    if lists_unordered:
        def with_sorted_table(lines):
            at = [i for i, l in enumerate(lines) if l.startswith("sequence:")]
            assert at and at == list(range(at[0], at[-1] + 1))
            return lines[:at[0]] + sorted(lines[at[0]:at[-1] + 1]) + lines[at[-1] + 1:]
        got, exp = with_sorted_table(got), with_sorted_table(exp)
    for i, (g, e) in enumerate(zip(got, exp)):
        if volatile(e):
            assert volatile(g)
        else:
            assert g == e, (tag, i, g[:300], e[:300])


def run_mcq(files, args, out, device):
    build.build_library()
    env = dict(os.environ)
    env["MCQ_PROFILE"] = "1"
    env.pop("MCQ_FORMAT_DEVICE", None)
    if device:
        env["MCQ_FORMAT_DEVICE"] = "1"
    cmd = [build.MCQ, "query", "toy32"] + files + args + ["-threads", "1", "-out", str(out)]
    r = subprocess.run(cmd, cwd=GOLD, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr
    return out.read_text().split("\n"), r.stderr


def library_calls(stderr):
    """-> [(calls, reads, lines, batches on the host)] of every job the run reported"""
    found = re.findall(r"mapping lines on the device: (\d+) mc_format_mappings calls, (\d+) reads, (\d+) lines, (\d+) batches formatted on the host", stderr)
    assert found, stderr
    return [tuple(int(x) for x in m) for m in found]


def reads_of_summary(lines):
    """the reads (pairs) a run classified or did not: the summary's unclassified count plus the classified ones up to the highest rank"""
    start = next(i for i, l in enumerate(lines) if re.match(r"^(?:# |%%)(unclassified:|classified:)", l))
    block = []
    for l in lines[start:]:
        m = re.match(r"^(?:# |%%)(unclassified:|  \w+) +[-+.\de]+% \((\d+)\)$", l)
        if m:
            block.append((m.group(1), int(m.group(2))))
        elif block and not re.match(r"^(?:# |%%)classified:", l):
            break
    assert block
    return sum(n for k, n in block if k == "unclassified:") + max([n for k, n in block if k != "unclassified:"] or [0])


def mapping_lines(lines, comment="# "):
    return [l for l in lines if l and not l.startswith(comment)]


@pytest.mark.parametrize("case", DEVICE_CASES)
def test_golden_cases_through_the_library(case, tmp_path):
    c = cli_case(case)
    got, stderr = run_mcq(c["files"], c["args"], tmp_path / "out.txt", device=True)
    same_lines(got, c["lines"], case, lists_unordered="-hits-per-ref" in c["args"])
    (calls, reads, lines, on_host), = library_calls(stderr)
    comment = c["args"][c["args"].index("-comment") + 1] if "-comment" in c["args"] else "# "
    body = mapping_lines(c["lines"], comment)
    if case in ("hits_per_ref_lineage", "abundances_species"):        # (the targets' lists / the abundance table follow the mapping lines)
        body = [l for l in body if re.match(r"^(\d+\t\|\t)?(read\d+|pair\d+/[12])\t", l)]
    assert calls > 0 and on_host == 0 and lines == len(body) > 0
    assert reads == reads_of_summary(c["lines"]) >= lines             # every read went through the library


def test_format_matrix_in_one_interactive_session(tmp_path):
    build.build_library()
    c = cli_case("format_matrix")
    assert len(c["matrix"]) == 144
    stdin = ""
    for i, line in enumerate(c["matrix"]):
        stdin += " ".join(["cli_fmt.fa"] + line + ["-out", str(tmp_path / f"fmt{i}.txt")]) + "\n"
    env = dict(os.environ, MCQ_PROFILE="1", MCQ_FORMAT_DEVICE="1")
    r = subprocess.run([build.MCQ, "query", "toy32", "-threads", "1"], cwd=GOLD, input=stdin + "\n", capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr
    for i, exp in enumerate(c["outputs"]):
        same_lines(open(tmp_path / f"fmt{i}.txt").read().split("\n"), exp, ("format_matrix", i, c["matrix"][i]))
    jobs = library_calls(r.stderr)
    assert len(jobs) == 144
    for (calls, reads, lines, on_host), exp in zip(jobs, c["outputs"]):
        assert calls > 0 and reads == 30 and on_host == 0 and lines == len(mapping_lines(exp))


@pytest.mark.parametrize("case", sorted(HOST_CASES))
def test_what_the_library_does_not_print_keeps_the_host_loop_and_says_so(case, tmp_path):
    c = cli_case(case)
    got, stderr = run_mcq(c["files"], c["args"], tmp_path / "out.txt", device=True)
    same_lines(got, c["lines"], case)
    assert "mapping lines on the device" not in stderr
    m = re.search(r"mcq: mapping lines formatted on the host \((.*)\)", stderr)
    assert m and HOST_CASES[case] in m.group(1), stderr


def test_without_the_switch_no_word_about_it(tmp_path):
    c = cli_case("hitdiff_percent")
    got, stderr = run_mcq(c["files"], c["args"], tmp_path / "out.txt", device=False)
    same_lines(got, c["lines"], "hitdiff_percent")
    assert "mapping lines" not in stderr and "mc_format" not in stderr
