"""CPU: the query path's hand-over rule (csrc/read_class.h: read_class, filter_takes, filter_second, segment_hits, the work-list record,
the classes' counter slots) against the decision table of tests/cpp/read_class_check.cpp -- a stand-alone host program, built and run
under the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_read_class_rule_limits_and_record_under_sanitizers(tmp_path):
    exe = str(tmp_path / "read_class_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "metacache_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "read_class_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "MISMATCH" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    for part in ("rule ok: 11070 cases", "limits ok: 11070 cases", "record ok: 30 cases", "slots ok: 7 cases"):
        assert part in r.stdout, r.stdout[-2000:]
