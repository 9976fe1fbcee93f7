"""Shared pieces of the generated-circuit tests (tests/test_circuits.py, tests/test_cpp_surface.py):
the one build and run of the host conformance program tests/cpp/test_circuits.cpp, and the
description of the 14 circuits of binius-ntt_amd/csrc/bitsliced_gen.hpp with their expected values
from the oracle (test infrastructure only)."""
import functools
import os
import subprocess
import time
from collections import namedtuple

import numpy as np

import _oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = "/opt/rocm"
CSRC = os.path.join(ROOT, "binius-ntt_amd", "csrc")
GEN_HEADER = os.path.join(CSRC, "bitsliced_gen.hpp")
CIRCUITS_BIN = os.path.join(ROOT, "tests", "cpp", "build", "test_circuits")

# groups x 2^h bits per element of a and out; the second operand is one GF(2^(2^h)) value that
# multiplies every group: bitsliced (2^h words, one value per bit-lane) or compact (one value per
# block; `uniform`: one per 64 blocks on the device). Order = bitsliced_gen.hpp = bn_circuit_device.
Spec = namedtuple("Spec", "name groups h compact acc alias uniform")
SPECS = (
    Spec("bsm2_mul", 1, 2, False, False, True, False), Spec("bsm3_mul", 1, 3, False, False, True, False),
    Spec("bsm3x4_fma_tw", 4, 3, True, True, False, False), Spec("bsm3x4_mul_acc", 4, 3, False, True, False, False),
    Spec("bsm4_mul", 1, 4, False, False, True, False), Spec("bsm4x2_fma_tw", 2, 4, True, True, False, False),
    Spec("bsm4x2_mul_acc", 2, 4, False, True, False, False), Spec("bsm5_mul", 1, 5, False, False, True, False),
    Spec("bsm5_fma_tw", 1, 5, True, True, False, False), Spec("bsm5_mul_acc", 1, 5, False, True, False, False),
    Spec("bsm6_mul", 1, 6, False, False, True, False), Spec("bsm7_mul", 1, 7, False, False, True, False),
    Spec("bsm5_mul_w", 1, 5, True, False, False, True), Spec("bsm6_fma_w2", 1, 6, True, True, False, True),
)


@functools.lru_cache(maxsize=None)
def host_conformance():
    """Builds tests/cpp/test_circuits.cpp (once per session) and runs it. Returns (returncode,
    output lines, compile seconds, run seconds)."""
    os.makedirs(os.path.dirname(CIRCUITS_BIN), exist_ok=True)
    oracle = O.ORACLE_DIR
    O.lib()  # builds liboracle.so when it is missing
    t0 = time.time()
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROCM, "include"), "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "test_circuits.cpp"), "-o", CIRCUITS_BIN,
                           "-L", oracle, "-loracle", "-Wl,-rpath," + oracle])
    t1 = time.time()
    p = subprocess.run([CIRCUITS_BIN], capture_output=True, text=True, timeout=300)
    t2 = time.time()
    print("test_circuits: compile %.1f s, run %.2f s" % (t1 - t0, t2 - t1))
    return p.returncode, (p.stdout + p.stderr).splitlines(), t1 - t0, t2 - t1


# ---------------------------------------------------------------- expected values
def omul(a, b, h):
    return O.mul128(a, b) if h == 7 else O.mul(a, b, h)


def expect(spec, a, b, o):
    """b times each 2^h-bit coordinate of a, on top of the accumulator (python ints)."""
    w = 1 << spec.h
    m = (1 << w) - 1
    r = o if spec.acc else 0
    for g in range(spec.groups):
        r ^= omul((a >> (w * g)) & m, b, spec.h) << (w * g)
    return r


def bitslice(elems, bits):
    """(n, 32) python ints -> (n, bits) uint32 words: word i of a block = bit i of its 32 elements."""
    n = len(elems)
    limbs = (bits + 31) // 32
    e = np.array([[[(x >> (32 * l)) & 0xFFFFFFFF for l in range(limbs)] for x in blk] for blk in elems], dtype=np.uint64)
    i = np.arange(bits)
    bit = (e[:, :, i // 32] >> (i % 32).astype(np.uint64)) & np.uint64(1)  # (n, 32, bits)
    words = (bit << np.arange(32, dtype=np.uint64)[None, :, None]).sum(axis=1)
    return words.astype(np.uint32).reshape(n, bits)


def unbitslice(words, bits):
    """(n, bits) uint32 words -> (n, 32) python ints."""
    w = np.asarray(words, dtype=np.uint64).reshape(-1, bits)
    bit = (w[:, :, None] >> np.arange(32, dtype=np.uint64)[None, None, :]) & np.uint64(1)  # (n, bits, 32)
    out = []
    for blk in bit:
        vals = [0] * 32
        for l in range(0, bits, 32):
            k = min(32, bits - l)
            limb = (blk[l:l + k] << np.arange(k, dtype=np.uint64)[:, None]).sum(axis=0)
            for e in range(32):
                vals[e] |= int(limb[e]) << l
        out.append(vals)
    return out
