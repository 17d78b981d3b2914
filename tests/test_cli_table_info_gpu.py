"""GPU: `mcq info <db> statistics | featurecounts | featuremap` behind MCQ_INFO_DEVICE=1 against the reference's recorded stdout."""
import os
import subprocess

import pytest

import table_info_ref as ref
from metacache_amd import build

pytestmark = pytest.mark.gpu


def run_info(args, **env):
    build.build_library()
    return subprocess.run([build.MCQ, "info"] + args, cwd=ref.GOLD, capture_output=True, text=True, timeout=300, env=dict(os.environ, MCQ_INFO_DEVICE="1", **env))


@pytest.mark.parametrize("case", sorted(ref.golden()))
def test_info_of_the_tables_content_matches_reference(case):
    """identical except the program version line; the lines between the two rules are compared as a sorted set within their part (the
    reference walks its own hash slots, mcq prints ascending features), the `database part N:` headers stay in place"""
    c = ref.golden()[case]
    r = run_info(c["args"])
    assert r.returncode == 0, r.stderr
    got, exp = ref.canonical(r.stdout.split("\n")), ref.canonical(c["stdout"])
    assert got == exp, (case, [(g, e) for g, e in zip(got, exp) if g != e][:5], len(got), len(exp))
    _, parts, _ = ref.split_output(ref.drop_version(r.stdout.split("\n")))
    for _, lines in parts:                                                  # mcq's own order: ascending features
        feats = [int(l.split(" -> ")[0]) for l in lines]
        assert feats == sorted(feats)


@pytest.mark.parametrize("alias,topic", [("stat", "statistics"), ("loc", "featuremap"), ("locations", "featuremap"), ("features", "featuremap")])
def test_topic_aliases(alias, topic):
    r = run_info(["toy32p2", alias], MCQ_PROFILE="1")
    assert r.returncode == 0, r.stderr
    assert ref.canonical(r.stdout.split("\n")) == ref.canonical(ref.golden()[topic + "_toy32p2"]["stdout"])
    assert "mcq profile: table info: mc_table_histogram 2 calls" in r.stderr
