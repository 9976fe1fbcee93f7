"""The bit-reversal permutation and the verifier's leaf fold of the C++ mirror
(tests/cpp/test_bitrev.cpp): builds against the C-ABI alone (CPU) and, on the GPU, checks bit_reverse
at log_n = 7 and 13 against the index permutation, fri_fold_leaf against fri_fold at (12, 1, round 0,
arity 4), and the argument errors."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "binius-ntt_amd", "lib")
ORACLE = os.path.join(ROOT, "oracle")
BIN = os.path.join(ROOT, "tests", "cpp", "build", "test_bitrev")


def _build():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "binius-ntt_amd", "host", "ulvt"),
                           os.path.join(ROOT, "tests", "cpp", "test_bitrev.cpp"), "-o", BIN,
                           "-L", LIBDIR, "-lbinius_ntt_amd", "-L", ORACLE, "-loracle",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath," + ORACLE, "-Wl,--allow-shlib-undefined"])


def test_cpp_bitrev_builds_against_the_c_abi():
    _build()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_cpp_bitrev_properties():
    _build()
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    out = p.stdout.splitlines()
    assert p.returncode == 0, p.stdout + p.stderr
    assert not [l for l in out if l.startswith("FAIL")]
    # 2 sizes x 3 properties, the leaf folds, and the three argument checks
    assert len([l for l in out if l.startswith("ok ")]) == 10
