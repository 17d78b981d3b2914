"""CPU: the table's load-time size rule, the multi-part merge and Mode T's cut (csrc/table_rules.h) against the
naive model of tests/cpp/table_rules_check.cpp -- a stand-alone host program, built and run under the address and undefined-behaviour
sanitizers: the merge re-homes buckets inside std::vectors with index arithmetic of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_table_rules_merge_and_cut_under_sanitizers(tmp_path):
    exe = str(tmp_path / "table_rules_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "metacache_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "table_rules_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "MISMATCH" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    for part in ("rules ok: 64 settings", "merge ok: 77 cases", "cut ok: 60 cases"):
        assert part in r.stdout, r.stdout[-2000:]
