"""CPU (needs g++ only): the two file formats of the BayesHammer stage on the host.

tests/hammer_files_check.cpp is a stand-alone program over csrc/hammer_files.h, the host-only header that packs and
unpacks binary_write(KMerStat) records (bbk_kmerstats_write / _load, bbk_subclusters_write) and brings a cluster listing
into the documented order (bbk_hamclusters_load).  Built with AddressSanitizer + UBSan (host code only, nothing is
loaded into python) and run once."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hammer_files_on_the_host(tmp_path):
    exe = str(tmp_path / "hammer_files_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "hammer_files_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), timeout=120)
    assert r.returncode == 0 and "HAMMER-FILES-OK" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
