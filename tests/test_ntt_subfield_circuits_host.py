"""The register-tile passes' small-sub-field circuits (binius-ntt_amd/csrc/bitsliced_ntt_gen.hpp:
bsm2x8_fma_tw on the 8 GF(2^4) coordinates of a limb, bsm1x16_fma_tw on its 16 GF(2^2) coordinates)
on the host: the stand-alone program tests/cpp/test_ntt_subfield_circuits.cpp, built with
AddressSanitizer + UBSan as tests/test_ntt_circuits_host.py builds its program, runs them through
the conformance routines of circuit_conformance.hpp against the oracle (random, edge, every basis
pair, accumulation into out) and checks that a GF(2^4) / GF(2^2) twiddle gives the same result
through bsm3x4_fma_tw. That the committed header is the generator's output is checked in
tests/test_ntt_circuits_host.py; on the device the circuits run in
tests/test_gpu_ntt_subfield_stages.py."""
import os
import re
import subprocess

import _circuits as C
import _oracle as O

NTT_HEADER = os.path.join(C.CSRC, "bitsliced_ntt_gen.hpp")
BIN = os.path.join(C.ROOT, "tests", "cpp", "build", "test_ntt_subfield_circuits")
CLANG = os.path.join(C.ROCM, "llvm", "bin", "clang++")


def test_subfield_circuits_cost_what_the_design_counts():
    # DESIGN.md section 5.2 / 5.3 count the first pass's instructions with these
    with open(NTT_HEADER) as f:
        text = f.read()
    for name, insts in (("bsm2x8_fma_tw", 202), ("bsm1x16_fma_tw", 116)):
        body = re.search(r"void %s\([^)]*\) \{\n(.*?)^\}$" % name, text, re.M | re.S).group(1)
        assert len(re.findall(r"^\tconst uint32_t t\d+ = ", body, re.M)) == insts, name


def test_subfield_circuits_conform_on_host_under_sanitizers():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    oracle = O.ORACLE_DIR
    O.lib()  # builds liboracle.so when it is missing
    # -fno-inline: see tests/cpp/Makefile (the host form of BN_BITOP3 stays a call)
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fno-inline",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(C.ROCM, "include"), "-I", C.CSRC,
                           os.path.join(C.ROOT, "tests", "cpp", "test_ntt_subfield_circuits.cpp"), "-o", BIN,
                           "-L", oracle, "-loracle", "-Wl,-rpath," + oracle])
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    lines = (p.stdout + p.stderr).splitlines()
    assert not [l for l in lines if l.startswith("FAIL")], "\n".join(l for l in lines if l.startswith("FAIL"))
    assert p.returncode == 0, "\n".join(lines[-20:])
    ok = {tuple(l.split()[1:3]) for l in lines if l.startswith("ok ")}
    for name in ("bsm2x8_fma_tw", "bsm1x16_fma_tw"):
        for check in ("random", "edge", "basis", "accumulate", "identity"):
            assert (name, check) in ok, "no ok line for %s %s" % (name, check)
