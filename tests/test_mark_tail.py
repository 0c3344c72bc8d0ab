"""CPU (needs g++ only): the rank-of-a-position helper of the mark-bit scatter tail on the host.

tests/mark_tail_check.cpp is a stand-alone program over csrc/msd_mark_tail.h, the layout and index arithmetic that
k_part_reads_narrow, k_part_view_lt and k_part_lt2 share: synthetic run tables and bucket spans, every position against a
naive scan.  Built once plain and once with AddressSanitizer + UBSan (host code only, nothing is loaded into python)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan-ubsan"])
def test_mark_tail_on_the_host(tmp_path, flags):
    exe = str(tmp_path / "mark_tail_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags +
                          ["-o", exe, os.path.join(ROOT, "tests", "mark_tail_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), timeout=120)
    assert r.returncode == 0 and "MARK-CHECK-OK" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
