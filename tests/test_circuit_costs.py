"""Gate counts of the generated circuits (binius-ntt_amd/tools/gen_bitsliced.py): none of the 14
of bitsliced_gen.hpp may cost more instructions than it did before the NTT passes got their own
re-packed GF(2^32) circuits, and those, which the generator writes to
bitsliced_ntt_gen.hpp and which stand in the passes where bsm5_mul (1022) and bsm5_mul_w (1053)
stood, must stay strictly below them: the headline transform spends 82 % of its bottom pass
there. The conformance of the circuits themselves is tests/test_circuits.py and
tests/test_ntt_circuits_host.py."""
import os
import re
import subprocess
import sys

import _circuits as C

GENERATOR = os.path.join(C.ROOT, "binius-ntt_amd", "tools", "gen_bitsliced.py")
# header order: the counts before the re-packing
BEFORE = [25, 93, 342, 331, 316, 606, 583, 1022, 1085, 1038, 3155, 9712, 1053, 3276]


def test_no_circuit_costs_more_and_bsm5_mul_costs_less(tmp_path):
    out = tmp_path / "bitsliced_gen.hpp"
    env = {k: v for k, v in os.environ.items() if not k.startswith("BN_GEN_")}  # the defaults
    p = subprocess.run([sys.executable, GENERATOR, "-o", str(out)], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr
    printed = [int(m.group(1)) for m in re.finditer(r"^\(\d+, '[^']+', (\d+)\)$", p.stderr, re.M)]
    names = [s.name for s in C.SPECS]
    assert len(printed) == len(names) == len(BEFORE)
    # the printed counts are the bodies' (test_circuits.py checks that on the committed header too)
    found = re.findall(r"^__host__ __device__ __forceinline__ void (\w+)\([^)]*\) \{\n(.*?)^\}$", out.read_text(), re.M | re.S)
    assert [f[0] for f in found] == names
    assert [len(re.findall(r"^\tconst uint32_t t\d+ = ", body, re.M)) for _, body in found] == printed
    worse = ["%s %d > %d" % (n, got, was) for n, got, was in zip(names, printed, BEFORE) if got > was]
    assert not worse, worse
    ntt = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"^ntt (\w+) (\d+)$", p.stderr, re.M))
    text = (tmp_path / "bitsliced_ntt_gen.hpp").read_text()
    for name in ("ntt_mul32", "ntt_mul32_w"):
        body = re.search(r"void %s\([^)]*\) \{\n(.*?)^\}$" % name, text, re.M | re.S).group(1)
        assert len(re.findall(r"^\tconst uint32_t t\d+ = ", body, re.M)) == ntt[name], name
    assert ntt["ntt_mul32"] < printed[names.index("bsm5_mul")] <= 1022
    assert ntt["ntt_mul32_w"] < printed[names.index("bsm5_mul_w")] <= 1053
