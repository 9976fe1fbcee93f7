// Conformance checks for the 14 generated bitsliced multiply circuits (binius-ntt_amd/csrc/
// bitsliced_gen.hpp) on the host, shared by tests/cpp/test_circuits.cpp and the sanitizer program
// tests/cpp/test_host_asan.cpp. Include it in ONE translation unit per program: it instantiates
// every circuit exactly once (invoke() below), which is most of the program's compile time.
//
// The expected value always comes from the oracle's compact tower product (orc_mul, orc_mul128,
// oracle/tower.c), never from another circuit. Every operand lives in its own heap allocation of
// exactly the documented size, so an emitter that indexes past an operand is an AddressSanitizer
// report in the sanitizer build.
//
// A circuit is described by: the bits of an element of `a` (= words of a and out), the number of
// sub-field coordinates G the second operand acts on and their height h (bits = G * 2^h), whether
// the second operand is bitsliced (2^h words, one element per bit-lane) or compact (one value for
// the block), and whether out is accumulated into. Per check one line is printed:
//   ok <circuit> <check> (<calls> calls)      or      FAIL <circuit> <check> ...
// Checks: random, edge, basis, identity, and alias for the alias-safe bsmH_mul.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "bitsliced_gen.hpp"

extern "C" {
void orc_init(void);
uint64_t orc_mul(uint64_t a, uint64_t b, int h);
void orc_mul128(const uint32_t a[4], const uint32_t b[4], uint32_t out[4]);
}

namespace conformance {

typedef unsigned __int128 u128;

struct Spec {
	const char* name;
	int groups;    // sub-field coordinates of an element that the second operand multiplies
	int h;         // their tower height
	bool compact;  // second operand: one compact value (true) or 2^h bitsliced words (false)
	bool acc;      // out ^= product (true) or out = product (false)
	bool alias;    // out may be any operand (the bsmH_mul promise)
};

// the order of bitsliced_gen.hpp; bn_circuit_device() numbers the circuits the same way
static const Spec kSpecs[14] = {
	{"bsm2_mul", 1, 2, false, false, true},        {"bsm3_mul", 1, 3, false, false, true},
	{"bsm3x4_fma_tw", 4, 3, true, true, false},    {"bsm3x4_mul_acc", 4, 3, false, true, false},
	{"bsm4_mul", 1, 4, false, false, true},        {"bsm4x2_fma_tw", 2, 4, true, true, false},
	{"bsm4x2_mul_acc", 2, 4, false, true, false},  {"bsm5_mul", 1, 5, false, false, true},
	{"bsm5_fma_tw", 1, 5, true, true, false},      {"bsm5_mul_acc", 1, 5, false, true, false},
	{"bsm6_mul", 1, 6, false, false, true},        {"bsm7_mul", 1, 7, false, false, true},
	{"bsm5_mul_w", 1, 5, true, false, false},      {"bsm6_fma_w2", 1, 6, true, true, false},
};

inline int a_bits(const Spec& s) { return s.groups << s.h; }
inline int b_bits(const Spec& s) { return 1 << s.h; }

// The one call site of every circuit. w is the compact operand of the forms that take one.
static void invoke(int id, const uint32_t* a, const uint32_t* b, uint64_t w, uint32_t* out) {
	switch (id) {
		case 0: bn::bsm2_mul(a, b, out); break;
		case 1: bn::bsm3_mul(a, b, out); break;
		case 2: bn::bsm3x4_fma_tw(a, (uint32_t)w, out); break;
		case 3: bn::bsm3x4_mul_acc(a, b, out); break;
		case 4: bn::bsm4_mul(a, b, out); break;
		case 5: bn::bsm4x2_fma_tw(a, (uint32_t)w, out); break;
		case 6: bn::bsm4x2_mul_acc(a, b, out); break;
		case 7: bn::bsm5_mul(a, b, out); break;
		case 8: bn::bsm5_fma_tw(a, (uint32_t)w, out); break;
		case 9: bn::bsm5_mul_acc(a, b, out); break;
		case 10: bn::bsm6_mul(a, b, out); break;
		case 11: bn::bsm7_mul(a, b, out); break;
		case 12: bn::bsm5_mul_w(a, (uint32_t)w, out); break;
		default: bn::bsm6_fma_w2(a, (uint32_t)w, (uint32_t)(w >> 32), out); break;
	}
}

inline u128 mask(int bits) { return bits >= 128 ? ~(u128)0 : (((u128)1 << bits) - 1); }

// the oracle's product in GF(2^(2^h)), 0 <= h <= 7
inline u128 omul(u128 a, u128 b, int h) {
	if (h <= 6) return orc_mul((uint64_t)(a & mask(1 << h)), (uint64_t)(b & mask(1 << h)), h);
	uint32_t x[4], y[4], z[4];
	for (int i = 0; i < 4; i++) x[i] = (uint32_t)(a >> (32 * i)), y[i] = (uint32_t)(b >> (32 * i));
	orc_mul128(x, y, z);
	return (u128)z[0] | ((u128)z[1] << 32) | ((u128)z[2] << 64) | ((u128)z[3] << 96);
}

// b times each 2^eh-bit coordinate of a (bits wide), on top of o
inline u128 expect(int bits, int eh, u128 a, u128 b, u128 o) {
	u128 r = o;
	for (int c = 0; c < bits; c += 1 << eh) r ^= omul(a >> c, b, eh) << c;
	return r;
}

struct Rng {  // splitmix64
	uint64_t s;
	uint64_t next() {
		uint64_t z = (s += 0x9E3779B97F4A7C15ull);
		z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
		z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
		return z ^ (z >> 31);
	}
	u128 bits(int n) { return (((u128)next() << 64) | next()) & mask(n); }
	u128 nonzero(int n) {
		const u128 v = bits(n);
		return v ? v : 1;
	}
};

// One call's operands as 32 compact elements each. For a compact second operand every b[e] holds
// the same value. o is the initial content of out (the accumulator, or garbage that a plain
// multiply has to overwrite).
struct Case {
	u128 a[32], b[32], o[32];
};

struct Buf {  // an operand in a heap allocation of exactly its size
	uint32_t* p;
	int n;
	explicit Buf(int words) : p(words ? (uint32_t*)malloc(sizeof(uint32_t) * (size_t)words) : nullptr), n(words) {}
	~Buf() { free(p); }
	Buf(const Buf&) = delete;
	Buf& operator=(const Buf&) = delete;
	void slice(const u128* el) {  // word i = bit i of the 32 elements
		for (int i = 0; i < n; i++) {
			uint32_t w = 0;
			for (int e = 0; e < 32; e++) w |= (uint32_t)((el[e] >> i) & 1u) << e;
			p[i] = w;
		}
	}
	u128 element(int e) const {
		u128 v = 0;
		for (int i = 0; i < n; i++) v |= (u128)((p[i] >> e) & 1u) << i;
		return v;
	}
};

enum Mode { DISTINCT = 0, OUT_IS_A = 1, OUT_IS_B = 2, SQUARE_IN_PLACE = 3 };

struct Tally {
	const char* circuit;
	const char* check;
	long calls = 0, fails = 0;
	Tally(const char* c, const char* k) : circuit(c), check(k) {}
	void fail(int mode, int e, const char* what, u128 got, u128 want) {
		if (fails++ < 4)
			printf("FAIL %s %s call %ld mode %d element %d %s: %016llx%016llx != %016llx%016llx\n", circuit, check, calls, mode, e,
			       what, (unsigned long long)(got >> 64), (unsigned long long)got, (unsigned long long)(want >> 64),
			       (unsigned long long)want);
	}
	int done() {
		if (!fails) printf("ok %s %s (%ld calls)\n", circuit, check, calls);
		else printf("FAIL %s %s: %ld wrong elements in %ld calls\n", circuit, check, fails, calls);
		fflush(stdout);
		return fails ? 1 : 0;
	}
};

// Runs circuit `id` once on `c` and compares every element with the oracle at height eh
// (eh = the circuit's own h, or another height for the sub-field identities). Operands that are
// not the destination must come back unchanged.
static void run_case(int id, const Case& c, int mode, int eh, Tally& t) {
	const Spec& s = kSpecs[id];
	const int na = a_bits(s), nb = s.compact ? 0 : b_bits(s);
	u128 want[32];
	for (int e = 0; e < 32; e++) {
		const u128 b = mode == SQUARE_IN_PLACE ? c.a[e] : c.b[e];
		want[e] = expect(na, eh, c.a[e], b, s.acc ? c.o[e] : 0);
	}
	Buf a(na), b(mode == SQUARE_IN_PLACE ? 0 : nb), o(mode == DISTINCT ? na : 0);
	a.slice(c.a);
	b.slice(c.b);
	o.slice(c.o);
	const uint32_t* pb = mode == SQUARE_IN_PLACE ? a.p : b.p;
	uint32_t* po = mode == DISTINCT ? o.p : mode == OUT_IS_B ? b.p : a.p;
	const uint64_t w = s.compact ? (uint64_t)c.b[0] : 0;
	invoke(id, a.p, pb, w, po);
	t.calls++;
	const Buf& out = mode == DISTINCT ? o : mode == OUT_IS_B ? b : a;
	for (int e = 0; e < 32; e++) {
		const u128 got = out.element(e);
		if (got != want[e]) t.fail(mode, e, "out", got, want[e]);
		if (mode != OUT_IS_A && mode != SQUARE_IN_PLACE && a.element(e) != c.a[e]) t.fail(mode, e, "a changed", a.element(e), c.a[e]);
		if (nb && mode != OUT_IS_B && mode != SQUARE_IN_PLACE && b.element(e) != (c.b[e] & mask(nb)))
			t.fail(mode, e, "b changed", b.element(e), c.b[e]);
	}
}

// ---- operand blocks ----
enum Block { ZERO, ONES, SINGLE_BITS, RANDOM };
inline void fill(u128* el, Block kind, int bits, int rot, Rng& r) {
	for (int e = 0; e < 32; e++)
		el[e] = kind == ZERO ? 0 : kind == ONES ? mask(bits) : kind == SINGLE_BITS ? (u128)1 << ((e + rot) % bits) : r.bits(bits);
}

inline void fill_compact(u128* el, u128 w) {
	for (int e = 0; e < 32; e++) el[e] = w;
}

// compact edge values of `bits` bits: 0, 1, all-ones, every single bit, and values with a zero
// byte (a zero nibble for an 8-bit value) between non-zero ones
static std::vector<u128> compact_edges(int bits, Rng& r) {
	std::vector<u128> v = {0, 1, mask(bits)};
	for (int i = 0; i < bits; i++) v.push_back((u128)1 << i);
	const int hole = bits > 8 ? 8 : 4;
	for (int at = 0; at < bits; at += hole) {
		v.push_back(mask(bits) & ~(mask(hole) << at));
		v.push_back((r.bits(bits) | ((u128)0x11 << (at ? 0 : hole))) & ~(mask(hole) << at) & mask(bits));
	}
	return v;
}

static int check_random(int id, int trials, const int* modes, int n_modes, const char* label, Rng& r) {
	const Spec& s = kSpecs[id];
	Tally t(s.name, label);
	for (int m = 0; m < n_modes; m++)
		for (int trial = 0; trial < trials; trial++) {
			Case c;
			fill(c.a, RANDOM, a_bits(s), 0, r);
			if (s.compact) fill_compact(c.b, r.bits(b_bits(s)));
			else fill(c.b, RANDOM, b_bits(s), 0, r);
			for (int e = 0; e < 32; e++) c.o[e] = r.nonzero(a_bits(s));
			run_case(id, c, modes[m], s.h, t);
		}
	return t.done();
}

static int check_edge(int id, const int* modes, int n_modes, const char* label, Rng& r) {
	const Spec& s = kSpecs[id];
	Tally t(s.name, label);
	const int na = a_bits(s), nb = b_bits(s);
	struct Pick {
		Block kind;
		int rot;
	};
	const Pick picks[5] = {{ZERO, 0}, {ONES, 0}, {SINGLE_BITS, 0}, {SINGLE_BITS, 5}, {RANDOM, 0}};
	const std::vector<u128> ws = s.compact ? compact_edges(nb, r) : std::vector<u128>();
	const int n_b = s.compact ? (int)ws.size() : 5;
	for (int m = 0; m < n_modes; m++)
		for (int ia = 0; ia < 5; ia++)
			for (int ib = 0; ib < n_b; ib++) {
				Case c;
				fill(c.a, picks[ia].kind, na, picks[ia].rot, r);
				if (s.compact) fill_compact(c.b, ws[ib]);
				else fill(c.b, picks[ib].kind, nb, picks[ib].rot + 3, r);
				// the accumulator: non-zero random, and once per operand pair all-ones
				for (int e = 0; e < 32; e++) c.o[e] = r.nonzero(na);
				run_case(id, c, modes[m], s.h, t);
				if (s.acc) {
					fill(c.o, ONES, na, 0, r);
					run_case(id, c, modes[m], s.h, t);
				}
			}
	return t.done();
}

// e_i * e_j for every basis element e_i of a and e_j of the second operand, 32 pairs per call
// (bitsliced b) or 32 values of i per call and one j (compact w)
static int check_basis(int id, Rng& r) {
	const Spec& s = kSpecs[id];
	Tally t(s.name, "basis");
	const int na = a_bits(s), nb = b_bits(s);
	Case c;
	if (s.compact) {
		for (int j = 0; j < nb; j++)
			for (int i0 = 0; i0 < na; i0 += 32) {
				for (int e = 0; e < 32; e++) c.a[e] = (u128)1 << ((i0 + e) % na), c.o[e] = r.nonzero(na);
				fill_compact(c.b, (u128)1 << j);
				run_case(id, c, DISTINCT, s.h, t);
			}
	} else {
		for (int p0 = 0; p0 < na * nb; p0 += 32) {
			for (int e = 0; e < 32; e++) {
				const int p = (p0 + e) % (na * nb);
				c.a[e] = (u128)1 << (p / nb), c.b[e] = (u128)1 << (p % nb), c.o[e] = r.nonzero(na);
			}
			run_case(id, c, DISTINCT, s.h, t);
		}
	}
	return t.done();
}

// Sub-field identities. The kernels switch per stage between the GF(2^8) x 4, GF(2^16) x 2 and
// GF(2^32) circuits (fma_tw<FMAX> / mul_tw<FMAX>) and run GF(2^128) data limb by limb against
// GF(2^32) twiddles; both assume that an element of a sub-field acts on each coordinate of the
// tower representation on its own:
//  * the x4 / x2 forms equal o ^ orc_mul(a_e, w, 5) on the 32-bit elements of the limb, w
//    zero-extended (its bits above the sub-field are masked: the call sites pass zero there);
//  * every other circuit, with the second operand in the sub-field one level down (upper half
//    zero), equals the oracle's product at that lower height on each half.
static int check_identity(int id, int trials, Rng& r) {
	const Spec& s = kSpecs[id];
	Tally t(s.name, "identity");
	const int na = a_bits(s);
	const bool packed = s.groups > 1;
	const int sub = packed ? b_bits(s) : b_bits(s) / 2, eh = packed ? 5 : s.h - 1;
	std::vector<u128> ws = compact_edges(sub, r);
	for (int trial = 0; trial < trials; trial++) ws.push_back(r.bits(sub));
	for (size_t k = 0; k < ws.size(); k++) {
		Case c;
		fill(c.a, k % 7 == 3 ? SINGLE_BITS : RANDOM, na, (int)k, r);
		if (s.compact) fill_compact(c.b, ws[k]);
		else if (k < ws.size() - (size_t)trials) fill_compact(c.b, ws[k]);
		else fill(c.b, RANDOM, sub, 0, r);
		for (int e = 0; e < 32; e++) c.o[e] = r.nonzero(na);
		run_case(id, c, DISTINCT, eh, t);
	}
	return t.done();
}

// mul_tw's in-place sub-field use (antt_bs_dev.hpp): bsm3_mul(p + 8 g, W, p + 8 g) for g < 4 and
// bsm4_mul(p + 16 g, W, p + 16 g) for g < 2 on a 32-word limb p with W shared, against the
// GF(2^32) product by the zero-extended W.
static int check_in_place_groups(int id, int trials, Rng& r) {
	const Spec& s = kSpecs[id];
	Tally t(s.name, "identity-in-place");
	const int nb = b_bits(s), groups = 32 / nb;
	for (int trial = 0; trial < trials; trial++) {
		u128 a[32], w[32], want[32];
		fill(a, trial == 1 ? ONES : trial == 2 ? SINGLE_BITS : RANDOM, 32, trial, r);
		fill(w, trial == 0 ? ONES : trial == 3 ? SINGLE_BITS : RANDOM, nb, trial, r);
		for (int e = 0; e < 32; e++) want[e] = omul(a[e], w[e], 5);
		Buf p(32), W(nb);
		p.slice(a);
		W.slice(w);
		for (int g = 0; g < groups; g++) {
			invoke(id, p.p + nb * g, W.p, 0, p.p + nb * g);
			t.calls++;
		}
		for (int e = 0; e < 32; e++) {
			if (p.element(e) != want[e]) t.fail(OUT_IS_A, e, "out", p.element(e), want[e]);
			if (W.element(e) != w[e]) t.fail(OUT_IS_A, e, "W changed", W.element(e), w[e]);
		}
	}
	return t.done();
}

// Every check of every circuit; returns the number of failed checks. random_trials >= 64 is the
// conformance run; the sanitizer program passes a small count (it is after out-of-range reads,
// which do not depend on the data).
static int run_all(int random_trials, uint64_t seed = 12345) {
	orc_init();
	Rng r{seed};
	int failed = 0;
	const int distinct[1] = {DISTINCT}, aliased[3] = {OUT_IS_A, OUT_IS_B, SQUARE_IN_PLACE};
	for (int id = 0; id < 14; id++) {
		failed += check_random(id, random_trials, distinct, 1, "random", r);
		failed += check_edge(id, distinct, 1, "edge", r);
		failed += check_basis(id, r);
		failed += check_identity(id, random_trials, r);
		if (kSpecs[id].alias) {
			// accumulate forms are __restrict__: never called aliased
			int f = check_random(id, random_trials, aliased, 3, "alias", r);
			f += check_edge(id, aliased, 3, "alias-edge", r);
			failed += f;
		}
		if (id == 1 || id == 4) failed += check_in_place_groups(id, random_trials, r);
	}
	return failed;
}

}  // namespace conformance
