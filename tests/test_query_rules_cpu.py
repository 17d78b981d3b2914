"""CPU: the host's batch plan (csrc/query_rules.h: what the caller wants, the lane-path condition, the lane stage's order, the host's look at
the counters, what follows from them, the pipe's sketch sizes and the three filter pools) against the expressions it was gathered from,
kept flat in tests/cpp/query_rules_check.cpp as the model -- a stand-alone host program, built and run under the address and
undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_plan_equals_the_model_under_sanitizers(tmp_path):
    exe = str(tmp_path / "query_rules_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "metacache_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "query_rules_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "MISMATCH" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    for part in ("wants ok: 128 cases", "lane path ok: 1024 cases", "plan ok: 47775744 cases", "sketch sizes and pools ok: 1260 cases"):
        assert part in r.stdout, r.stdout[-2000:]
