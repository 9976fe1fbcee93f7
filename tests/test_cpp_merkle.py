"""The Merkle commitment of the C++ mirror (tests/cpp/test_merkle.cpp): builds against the C-ABI alone
(CPU) and, on the GPU, runs the mirror's flow at L = 7 and 13 against a tree built from the host-only
bn_merkle_hash_* calls, merkle_verify on records of the GPU's tree, and the argument errors."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "binius-ntt_amd", "lib")
ORACLE = os.path.join(ROOT, "oracle")
BIN = os.path.join(ROOT, "tests", "cpp", "build", "test_merkle")


def _build():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "binius-ntt_amd", "host", "ulvt"),
                           os.path.join(ROOT, "tests", "cpp", "test_merkle.cpp"), "-o", BIN,
                           "-L", LIBDIR, "-lbinius_ntt_amd", "-L", ORACLE, "-loracle",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath," + ORACLE, "-Wl,--allow-shlib-undefined"])


def test_cpp_merkle_builds_against_the_c_abi():
    _build()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_cpp_merkle_properties():
    _build()
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    out = p.stdout.splitlines()
    assert p.returncode == 0, p.stdout + p.stderr
    assert not [l for l in out if l.startswith("FAIL")]
    # 2 sizes x 3 properties, plus the nine argument checks
    assert len([l for l in out if l.startswith("ok ")]) == 15
