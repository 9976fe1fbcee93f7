// Host-side conformance of all 14 generated bitsliced multiply circuits (binius-ntt_amd/csrc/
// bitsliced_gen.hpp) against the oracle's compact tower product (orc_mul / orc_mul128,
// oracle/tower.c): random blocks, edge operands, every basis pair, the alias modes of the
// alias-safe multiplies and the sub-field identities the NTT kernels rely on. The checks are in
// circuit_conformance.hpp (shared with the sanitizer program test_host_asan.cpp). The circuits are
// __host__ __device__, so the host build runs exactly the gate list the kernels run; the device
// mappings of BN_BITOP3 / BN_BIT are covered by bn_circuit_device (tests/test_circuits.py).
// Prints one "ok <circuit> <check>" or "FAIL ..." line per circuit and check; exit status 0 iff
// every check passed.
#include "circuit_conformance.hpp"

int main() {
	const int failed = conformance::run_all(64);
	printf("%s: %d failed check(s)\n", failed ? "FAILED" : "PASSED", failed);
	return failed ? 1 : 0;
}
