// bn_sumcheck_interpolate: the round polynomial at the challenge, from its points (host only).
#include <string.h>

#include <utility>
#include "common.hpp"
#include "tower.hpp"

using namespace bn;

namespace {

// Interpolation on the nodes 0..n-1 (tower elements of GF(2^4)) by the coefficient form:
// c = V^-1 points with V[i][k] = i^k over GF(2^4), then p(r) = sum_k c_k r^k by Horner. V^-1 has
// GF(2^4) entries, and a GF(2^4) scalar times a GF(2^128) element acts on its 32 GF(2^4) coordinates
// (nibbles) one by one, so this is n^2 table-driven scalar products and n - 1 GF(2^128) products
// instead of the Lagrange form's n^2 GF(2^128) products (5.3 -> ~1 us for n = 4: on the host's
// critical path of every sumcheck round).
struct InterpTables {
	uint8_t vinv[17][16][16];  // [n][k][i]
	uint8_t smul[16][256];     // [c][byte]: the two GF(2^4) coordinates of the byte times c
	InterpTables() {
		for (int c = 0; c < 16; c++)
			for (int x = 0; x < 256; x++)
				smul[c][x] = (uint8_t)(tw_mul((uint64_t)c, (uint64_t)(x & 15), 2) | (tw_mul((uint64_t)c, (uint64_t)(x >> 4), 2) << 4));
		for (int n = 1; n <= 16; n++) {
			// Gauss-Jordan on [V | I] over GF(2^4); V is invertible (distinct nodes)
			uint8_t m[16][32] = {};
			for (int i = 0; i < n; i++) {
				uint64_t p = 1;
				for (int k = 0; k < n; k++) {
					m[i][k] = (uint8_t)p;
					p = tw_mul(p, (uint64_t)i, 2);
				}
				m[i][n + i] = 1;
			}
			for (int col = 0; col < n; col++) {
				int piv = col;
				while (m[piv][col] == 0) piv++;
				for (int k = 0; k < 2 * n; k++) std::swap(m[col][k], m[piv][k]);
				const uint64_t inv = tw_inv(m[col][col], 2);
				for (int k = 0; k < 2 * n; k++) m[col][k] = (uint8_t)tw_mul(m[col][k], inv, 2);
				for (int row = 0; row < n; row++) {
					if (row == col || m[row][col] == 0) continue;
					const uint64_t f = m[row][col];
					for (int k = 0; k < 2 * n; k++) m[row][k] ^= (uint8_t)tw_mul(f, m[col][k], 2);
				}
			}
			// V c = points  =>  c = V^-1 points; vinv[n][k][i] = (V^-1)[k][i]
			for (int k = 0; k < n; k++)
				for (int i = 0; i < n; i++) vinv[n][k][i] = m[k][n + i];
		}
	}
};

const InterpTables& interp_tables() {
	static const InterpTables t;
	return t;
}

}  // namespace

extern "C" int bn_sumcheck_interpolate(const uint32_t* points, int num_points, const uint32_t* challenge, uint32_t* out) {
	BN_CHECK_ARG(points && challenge && out, "NULL argument");
	BN_CHECK_ARG(num_points >= 1 && num_points <= 16, "num_points must be in [1, 16]");
	const InterpTables& T = interp_tables();
	const int n = num_points;
	// coefficients c_k = sum_i vinv[k][i] points_i (byte-wise scalar products)
	uint8_t c[16][16];
	for (int k = 0; k < n; k++) {
		uint8_t acc[16] = {};
		for (int i = 0; i < n; i++) {
			const uint8_t s = T.vinv[n][k][i];
			if (!s) continue;
			const uint8_t* pb = (const uint8_t*)(points + 4 * i);
			const uint8_t* tab = T.smul[s];
			for (int b = 0; b < 16; b++) acc[b] ^= tab[pb[b]];
		}
		memcpy(c[k], acc, 16);
	}
	auto ld = [](const uint8_t* p) {
		uint64_t lo, hi;
		memcpy(&lo, p, 8);
		memcpy(&hi, p + 8, 8);
		return bn::u128p{lo, hi};
	};
	const bn::u128p r{(uint64_t)challenge[0] | ((uint64_t)challenge[1] << 32), (uint64_t)challenge[2] | ((uint64_t)challenge[3] << 32)};
	bn::u128p acc = ld(c[n - 1]);
	for (int k = n - 2; k >= 0; k--) {
		acc = bn::tw_mul128_host(acc, r);
		const bn::u128p ck = ld(c[k]);
		acc.lo ^= ck.lo;
		acc.hi ^= ck.hi;
	}
	out[0] = (uint32_t)acc.lo;
	out[1] = (uint32_t)(acc.lo >> 32);
	out[2] = (uint32_t)acc.hi;
	out[3] = (uint32_t)(acc.hi >> 32);
	return BN_OK;
}

// bn_eq_eval: eq(a, b) = prod_i (a_i b_i ^ (1 ^ a_i)(1 ^ b_i)) (host only). In characteristic 2 the
// factor is 1 ^ a_i ^ b_i, so a variable costs the one product that accumulates it.
extern "C" int bn_eq_eval(int num_vars, const uint32_t* a, const uint32_t* b, uint32_t* out) {
	BN_CHECK_ARG(num_vars >= 0 && num_vars <= 128, "num_vars must be in [0, 128] (got %d)", num_vars);
	BN_CHECK_ARG(out != nullptr && ((a != nullptr && b != nullptr) || num_vars == 0), "NULL argument");
	auto ld = [](const uint32_t* p) { return bn::u128p{(uint64_t)p[0] | ((uint64_t)p[1] << 32), (uint64_t)p[2] | ((uint64_t)p[3] << 32)}; };
	bn::u128p acc{1, 0};
	for (int i = 0; i < num_vars; i++) {
		const bn::u128p x = ld(a + 4 * i), y = ld(b + 4 * i);
		// a b ^ (1 ^ a)(1 ^ b) = 1 ^ a ^ b (the two a b cancel)
		const bn::u128p f{1 ^ x.lo ^ y.lo, x.hi ^ y.hi};
		acc = bn::tw_mul128_host(acc, f);
	}
	out[0] = (uint32_t)acc.lo;
	out[1] = (uint32_t)(acc.lo >> 32);
	out[2] = (uint32_t)acc.hi;
	out[3] = (uint32_t)(acc.hi >> 32);
	return BN_OK;
}
