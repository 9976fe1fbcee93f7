"""The NTT passes' own GF(2^32) circuits (binius-ntt_amd/csrc/bitsliced_ntt_gen.hpp: ntt_mul32,
ntt_mul32_w) on the host: the committed header is what the generator writes, and the stand-alone
program tests/cpp/test_ntt_circuits.cpp, built with AddressSanitizer + UBSan, runs them through
the conformance routines of circuit_conformance.hpp against the oracle (random, edge, every basis
pair, sub-field identities, the alias modes of ntt_mul32). On the device they run in every NTT
test (tests/test_gpu_ntt_circuit_sites.py at the smallest sizes)."""
import os
import subprocess
import sys

import _circuits as C
import _oracle as O

NTT_HEADER = os.path.join(C.CSRC, "bitsliced_ntt_gen.hpp")
BIN = os.path.join(C.ROOT, "tests", "cpp", "build", "test_ntt_circuits")
CLANG = os.path.join(C.ROCM, "llvm", "bin", "clang++")


def test_committed_ntt_header_is_the_generators_output(tmp_path):
    out = tmp_path / "bitsliced_gen.hpp"
    p = subprocess.run([sys.executable, os.path.join(C.ROOT, "binius-ntt_amd", "tools", "gen_bitsliced.py"), "-o", str(out)],
                       capture_output=True, text=True, timeout=300,
                       env={k: v for k, v in os.environ.items() if not k.startswith("BN_GEN_")})  # the defaults
    assert p.returncode == 0, p.stderr
    with open(NTT_HEADER, "rb") as f:
        assert (tmp_path / "bitsliced_ntt_gen.hpp").read_bytes() == f.read()


def test_ntt_circuits_conform_on_host_under_sanitizers():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    oracle = O.ORACLE_DIR
    O.lib()  # builds liboracle.so when it is missing
    # -fno-inline: see tests/cpp/Makefile (the host form of BN_BITOP3 stays a call)
    subprocess.check_call([CLANG, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fno-inline",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(C.ROCM, "include"), "-I", C.CSRC,
                           os.path.join(C.ROOT, "tests", "cpp", "test_ntt_circuits.cpp"), "-o", BIN,
                           "-L", oracle, "-loracle", "-Wl,-rpath," + oracle])
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    lines = (p.stdout + p.stderr).splitlines()
    assert not [l for l in lines if l.startswith("FAIL")], "\n".join(l for l in lines if l.startswith("FAIL"))
    assert p.returncode == 0, "\n".join(lines[-20:])
    ok = {tuple(l.split()[1:3]) for l in lines if l.startswith("ok ")}
    for name, checks in (("bsm5_mul", ["random", "edge", "basis", "identity", "alias", "alias-edge"]),
                         ("bsm5_mul_w", ["random", "edge", "basis", "identity"])):
        for check in checks:
            assert (name, check) in ok, "no ok line for %s %s" % (name, check)
