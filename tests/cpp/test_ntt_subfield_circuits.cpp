// Host-side conformance of the two small-sub-field circuits of binius-ntt_amd/csrc/
// bitsliced_ntt_gen.hpp against the oracle's compact tower product:
//   bsm2x8_fma_tw   out ^= a * w on the 8 GF(2^4) coordinates of a 32-word limb, w in bits 0..3
//   bsm1x16_fma_tw  the same on the 16 GF(2^2) coordinates, w in bits 0..1
// They go through the routines of circuit_conformance.hpp that check bsm3x4_fma_tw (run_case and its
// operand blocks, edge values and tallies). Those routines reach a circuit through its name in
// invoke(), and run_case takes the height the oracle multiplies at: ids 2 and 5 (bsm3x4_fma_tw,
// bsm4x2_fma_tw: 32-word a, compact w, accumulating, as the new forms) are mapped onto the two new
// circuits after both generated headers have been read, and every case is run at height 2 / 1.
// The checks: random, edge, every basis pair, accumulation into out, and the identity the kernels
// rely on when they pick a stage's circuit by its class (antt_rr.hip): a GF(2^4) / GF(2^2) twiddle
// gives the same result through bsm3x4_fma_tw (the real one, called directly) and through the
// oracle's GF(2^32) product.
// Stand-alone program with its own main; tests/test_ntt_subfield_circuits_host.py builds it with
// AddressSanitizer + UBSan. Prints "ok <circuit> <check>" / "FAIL ..." lines; exit status 0 iff every
// check passed.
#include "bitsliced_gen.hpp"
#include "bitsliced_ntt_gen.hpp"
#define bsm3x4_fma_tw bsm2x8_fma_tw
#define bsm4x2_fma_tw bsm1x16_fma_tw
// invoke()'s other twelve call sites are never reached here: each is mapped onto the smallest circuit
// of its signature, so that this program does not compile the GF(2^32) .. GF(2^128) circuits under
// the sanitizers for nothing (tests/test_circuits.py and tests/test_asan.py run those)
namespace bn {
inline void unused_fma_w2(const uint32_t*, uint32_t, uint32_t, uint32_t*) {}
}
#define bsm3_mul bsm2_mul
#define bsm3x4_mul_acc bsm2_mul
#define bsm4_mul bsm2_mul
#define bsm4x2_mul_acc bsm2_mul
#define bsm5_mul bsm2_mul
#define bsm5_fma_tw bsm1x16_fma_tw
#define bsm5_mul_acc bsm2_mul
#define bsm6_mul bsm2_mul
#define bsm7_mul bsm2_mul
#define bsm5_mul_w bsm1x16_fma_tw
#define bsm6_fma_w2 unused_fma_w2
#include "circuit_conformance.hpp"
#undef bsm3x4_fma_tw

using namespace conformance;

struct Small {
	const char* name;
	int id;  // the conformance id whose call site runs the circuit
	int h;   // tower height of the twiddle: GF(2^(2^h))
};
static const Small kSmall[2] = {{"bsm2x8_fma_tw", 2, 2}, {"bsm1x16_fma_tw", 5, 1}};

static void random_acc(u128* o, Rng& r) {
	for (int e = 0; e < 32; e++) o[e] = r.nonzero(32);
}

static int check_random(const Small& s, int trials, Rng& r) {
	Tally t(s.name, "random");
	for (int trial = 0; trial < trials; trial++) {
		Case c;
		fill(c.a, RANDOM, 32, 0, r);
		fill_compact(c.b, r.bits(1 << s.h));
		random_acc(c.o, r);
		run_case(s.id, c, DISTINCT, s.h, t);
	}
	return t.done();
}

// a: zero, all-ones, single bits (two rotations), random; w: every value of the sub-field (16 / 4,
// which covers compact_edges' zero, one, all-ones and single bits); out: random and all-ones
static int check_edge(const Small& s, Rng& r) {
	Tally t(s.name, "edge");
	const Block kinds[5] = {ZERO, ONES, SINGLE_BITS, SINGLE_BITS, RANDOM};
	const int rots[5] = {0, 0, 0, 5, 0};
	std::vector<u128> ws = compact_edges(1 << s.h, r);
	for (int w = 0; w < (1 << (1 << s.h)); w++) ws.push_back((u128)w);
	for (int ia = 0; ia < 5; ia++)
		for (size_t iw = 0; iw < ws.size(); iw++) {
			Case c;
			fill(c.a, kinds[ia], 32, rots[ia], r);
			fill_compact(c.b, ws[iw]);
			random_acc(c.o, r);
			run_case(s.id, c, DISTINCT, s.h, t);
			fill(c.o, ONES, 32, 0, r);
			run_case(s.id, c, DISTINCT, s.h, t);
		}
	return t.done();
}

// e_i * e_j for every basis element e_i of the 32-bit limb (one per bit-lane) and e_j of the twiddle
static int check_basis(const Small& s, Rng& r) {
	Tally t(s.name, "basis");
	for (int j = 0; j < (1 << s.h); j++) {
		Case c;
		for (int e = 0; e < 32; e++) c.a[e] = (u128)1 << e;
		fill_compact(c.b, (u128)1 << j);
		random_acc(c.o, r);
		run_case(s.id, c, DISTINCT, s.h, t);
	}
	return t.done();
}

// out is accumulated into and nothing else: zero, all-ones and single-bit accumulators under a
// random product, and a zero twiddle leaves every accumulator as it was
static int check_accumulation(const Small& s, int trials, Rng& r) {
	Tally t(s.name, "accumulate");
	const Block kinds[4] = {ZERO, ONES, SINGLE_BITS, RANDOM};
	for (int trial = 0; trial < trials; trial++)
		for (int k = 0; k < 4; k++) {
			Case c;
			fill(c.a, RANDOM, 32, 0, r);
			fill_compact(c.b, trial == 0 ? (u128)0 : r.bits(1 << s.h));
			fill(c.o, kinds[k], 32, trial, r);
			run_case(s.id, c, DISTINCT, s.h, t);
		}
	return t.done();
}

// The same twiddle, zero-extended, through the circuit, through bsm3x4_fma_tw and through the
// oracle's GF(2^32) product (run_case at height 5): all three agree on every element.
static int check_identity(const Small& s, int trials, Rng& r) {
	Tally t(s.name, "identity");
	std::vector<u128> ws;
	for (int w = 0; w < (1 << (1 << s.h)); w++) ws.push_back((u128)w);
	for (int trial = 0; trial < trials; trial++) ws.push_back(r.bits(1 << s.h));
	for (size_t k = 0; k < ws.size(); k++) {
		Case c;
		fill(c.a, k % 7 == 3 ? SINGLE_BITS : RANDOM, 32, (int)k, r);
		fill_compact(c.b, ws[k]);
		random_acc(c.o, r);
		run_case(s.id, c, DISTINCT, 5, t);
		Buf a(32), o8(32);
		a.slice(c.a);
		o8.slice(c.o);
		bn::bsm3x4_fma_tw(a.p, (uint32_t)ws[k], o8.p);
		t.calls++;
		for (int e = 0; e < 32; e++) {
			const u128 want = expect(32, s.h, c.a[e], ws[k], c.o[e]);
			if (o8.element(e) != want) t.fail(DISTINCT, e, "bsm3x4_fma_tw", o8.element(e), want);
		}
	}
	return t.done();
}

int main() {
	orc_init();
	Rng r{20241};
	const int trials = 64;
	int failed = 0;
	for (const Small& s : kSmall) {
		failed += check_random(s, trials, r);
		failed += check_edge(s, r);
		failed += check_basis(s, r);
		failed += check_accumulation(s, trials, r);
		failed += check_identity(s, trials, r);
	}
	printf("%s: %d failed check(s)\n", failed ? "FAILED" : "PASSED", failed);
	return failed ? 1 : 0;
}
