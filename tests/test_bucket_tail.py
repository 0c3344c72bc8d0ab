"""CPU (needs g++ only): the copy-out step of k_bucket_dist_nb on the host.

tests/bucket_tail_check.cpp is a stand-alone program over csrc/msd_bucket_tail.h, the `__host__ __device__` helper the
kernel's tail calls per position: sorted buckets of 1 .. 5632 offsets, with and without one duplicate pair.  Built with
AddressSanitizer + UBSan (host code only, nothing is loaded into python) and run once."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bucket_tail_on_the_host(tmp_path):
    exe = str(tmp_path / "bucket_tail_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "bucket_tail_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), timeout=120)
    assert r.returncode == 0 and "TAIL-CHECK-OK" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
