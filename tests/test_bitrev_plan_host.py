"""CPU: the bit-reversal permutation's planner, address functions and LDS layout swept by a stand-alone
program (tests/cpp/test_bitrev_plan.cpp + binius-ntt_amd/csrc/bitrev_plan.cpp) built with
AddressSanitizer and UBSan: no library, no Python extension, no preload."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "binius-ntt_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "cpp", "build", "test_bitrev_plan")


def test_bitrev_plan_sweep_under_sanitizers():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "test_bitrev_plan.cpp"), os.path.join(CSRC, "bitrev_plan.cpp"),
                           "-o", BIN])
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert p.stdout.splitlines()[-1] == "PASSED (0 failures)"
