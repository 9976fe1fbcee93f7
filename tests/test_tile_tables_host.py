"""CPU: the tile-start tables of the additive NTT's pass kernels (closed-form outer offset, chunk
tables of the uniform twiddle parts) swept over all 95 plans by a stand-alone program
(tests/cpp/test_tile_tables.cpp + binius-ntt_amd/csrc/antt_passes.cpp) built with AddressSanitizer
and UBSan: no library, no Python extension, no preload."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "binius-ntt_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "cpp", "build", "test_tile_tables")
ROCM = "/opt/rocm"


def test_tile_tables_sweep_under_sanitizers():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROCM, "include"), "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "test_tile_tables.cpp"),
                           os.path.join(CSRC, "antt_passes.cpp"), "-o", BIN])
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    assert p.stdout.splitlines()[-1] == "PASSED (0 failures)"
