"""CPU: the reader of BayesHammer's config.info (host/hammer_config.hpp) on the shipped text (tests/golden/hammer_config.info,
a copy of configs/hammer/config.info: settings only) and on crafted ones, with AddressSanitizer + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hammer_config_reader(tmp_path):
    exe = str(tmp_path / "hammer_config_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "hammer_config_check.cpp")])
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "hammer_config.info")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "HAMMER-CONFIG-CHECK-OK" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
