"""CPU: the option table of the host tools (host/cli.hpp) on fixed argv arrays, with AddressSanitizer + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cli_option_table(tmp_path):
    exe = str(tmp_path / "cli_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cli_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "CLI-CHECK-OK" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
