"""Ring-switching of the C++ mirror (tests/cpp/test_ring_switch.cpp): builds against the C-ABI alone
(CPU) and, on the GPU, checks rs_partial_evals at log_n = 10 and gf128_linear_map (compact and
bitsliced) against the definitions bit by bit, the verifier's functions through the sumcheck's
identity, and the argument errors."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "binius-ntt_amd", "lib")
ORACLE = os.path.join(ROOT, "oracle")
BIN = os.path.join(ROOT, "tests", "cpp", "build", "test_ring_switch")


def _build():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "binius-ntt_amd", "host", "ulvt"),
                           os.path.join(ROOT, "tests", "cpp", "test_ring_switch.cpp"), "-o", BIN,
                           "-L", LIBDIR, "-lbinius_ntt_amd", "-L", ORACLE, "-loracle",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath," + ORACLE, "-Wl,--allow-shlib-undefined"])


def test_cpp_ring_switch_builds_against_the_c_abi():
    _build()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_cpp_ring_switch_properties():
    _build()
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    out = p.stdout.splitlines()
    assert p.returncode == 0, p.stdout + p.stderr
    assert not [l for l in out if l.startswith("FAIL")]
    # the partial evaluations and the four identities around them, two maps, four argument checks
    assert len([l for l in out if l.startswith("ok ")]) == 11
