// Host-side conformance of the two circuits of binius-ntt_amd/csrc/bitsliced_ntt_gen.hpp (ntt_mul32,
// ntt_mul32_w: the NTT passes' variants of bsm5_mul and bsm5_mul_w) against the oracle's compact
// tower product, through the routines of circuit_conformance.hpp. Those routines reach a circuit
// through its name in invoke(): the two names are mapped onto the variants below, after both
// generated headers have been read, so ids 7 and 12 run the variants (with bsm5_mul's alias modes
// and bsm5_mul_w's compact wave-uniform operand) and every other id its own circuit.
// Stand-alone program with its own main; tests/test_ntt_circuits_host.py builds it with
// AddressSanitizer + UBSan. Prints "ok <circuit> <check>" / "FAIL ..." lines (the names printed for
// ids 7 and 12 are the table's, bsm5_mul and bsm5_mul_w); exit status 0 iff every check passed.
#include "bitsliced_gen.hpp"
#include "bitsliced_ntt_gen.hpp"
#define bsm5_mul ntt_mul32
#define bsm5_mul_w ntt_mul32_w
#include "circuit_conformance.hpp"

int main() {
	using namespace conformance;
	orc_init();
	Rng r{20240};
	const int trials = 64;
	const int distinct[1] = {DISTINCT}, aliased[3] = {OUT_IS_A, OUT_IS_B, SQUARE_IN_PLACE};
	int failed = 0;
	for (int id : {7, 12}) {
		failed += check_random(id, trials, distinct, 1, "random", r);
		failed += check_edge(id, distinct, 1, "edge", r);
		failed += check_basis(id, r);
		failed += check_identity(id, trials, r);
		if (kSpecs[id].alias) {
			failed += check_random(id, trials, aliased, 3, "alias", r);
			failed += check_edge(id, aliased, 3, "alias-edge", r);
		}
	}
	printf("%s: %d failed check(s)\n", failed ? "FAILED" : "PASSED", failed);
	return failed ? 1 : 0;
}
