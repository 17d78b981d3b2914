"""CPU: the host rule that picks the instance of gw_filter_count_kernel<LOOKUP> for a batch (lookup_shape, csrc/query_rules.h) against the
list of shipped shape-fixed instances, kept in tests/cpp/lookup_shape_check.cpp -- a stand-alone host program, built and run under the
address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lookup_shape_equals_the_list_of_instances_under_sanitizers(tmp_path):
    exe = str(tmp_path / "lookup_shape_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "metacache_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "lookup_shape_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "MISMATCH" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    assert "lookup shape ok: 2840 cases, 8 fixed" in r.stdout, r.stdout[-2000:]
