// The verifier's side of ring-switching (host only: no plan, no device): the batching table
// B[u] = eq(r'', u), the row check of the partial evaluations s^, the sumcheck's claim s_0 from the
// transpose of s^ as a 128 x 128 bit matrix, and the tensor-algebra evaluation of the mapped eq
// column A~(rho). Elements are 4 little-endian words; bit v of an element is bit v % 32 of word
// v / 32 (beta_v, the bit basis of GF(2^128) over GF(2)).
#include "common.hpp"
#include "tower.hpp"

namespace bn {

static u128p rs_elem(const uint32_t* w) { return u128p{w[0] | ((uint64_t)w[1] << 32), w[2] | ((uint64_t)w[3] << 32)}; }

static void rs_store(uint32_t* out, u128p a) {
	out[0] = (uint32_t)a.lo;
	out[1] = (uint32_t)(a.lo >> 32);
	out[2] = (uint32_t)a.hi;
	out[3] = (uint32_t)(a.hi >> 32);
}

static u128p rs_xor(u128p a, u128p b) { return u128p{a.lo ^ b.lo, a.hi ^ b.hi}; }
static int rs_bit(u128p a, int v) { return (int)(((v < 64 ? a.lo : a.hi) >> (v & 63)) & 1); }
static u128p rs_beta(int v) { return v < 64 ? u128p{1ull << v, 0} : u128p{0, 1ull << (v - 64)}; }

// T[u] = prod_{i<7} (bit_i(u) ? r_i : 1 ^ r_i): variable i doubles the table, one product per pair
static void rs_eq7(const uint32_t* r, u128p* T) {
	T[0] = u128p{1, 0};
	for (int i = 0; i < 7; i++) {
		const u128p ri = rs_elem(r + 4 * i);
		for (int u = 0; u < (1 << i); u++) {
			const u128p hi = tw_mul128_host(T[u], ri);
			T[u + (1 << i)] = hi;
			T[u] = rs_xor(T[u], hi);
		}
	}
}

static u128p rs_dot(const u128p* a, const u128p* b) {
	u128p acc{0, 0};
	for (int u = 0; u < 128; u++) acc = rs_xor(acc, tw_mul128_host(a[u], b[u]));
	return acc;
}

}  // namespace bn

using namespace bn;

extern "C" int bn_rs_batch_table(const uint32_t* r2, uint32_t* out) {
	BN_CHECK_ARG(r2 != nullptr && out != nullptr, "NULL argument");
	u128p B[128];
	rs_eq7(r2, B);
	for (int u = 0; u < 128; u++) rs_store(out + 4 * u, B[u]);
	return BN_OK;
}

extern "C" int bn_rs_row_check(const uint32_t* shat, const uint32_t* r_low, uint32_t* out) {
	BN_CHECK_ARG(shat != nullptr && r_low != nullptr && out != nullptr, "NULL argument");
	u128p T[128], s[128];
	rs_eq7(r_low, T);
	for (int v = 0; v < 128; v++) s[v] = rs_elem(shat + 4 * v);
	rs_store(out, rs_dot(T, s));
	return BN_OK;
}

extern "C" int bn_rs_sumcheck_claim(const uint32_t* shat, const uint32_t* r2, uint32_t* out) {
	BN_CHECK_ARG(shat != nullptr && r2 != nullptr && out != nullptr, "NULL argument");
	u128p B[128], row[128];
	rs_eq7(r2, B);
	// row u = sum_v bit_u(s^_v) beta_v: the transpose of the bit matrix
	for (int u = 0; u < 128; u++) row[u] = u128p{0, 0};
	for (int v = 0; v < 128; v++) {
		const u128p sv = rs_elem(shat + 4 * v);
		for (int u = 0; u < 128; u++)
			if (rs_bit(sv, u)) row[u] = rs_xor(row[u], rs_beta(v));
	}
	rs_store(out, rs_dot(B, row));
	return BN_OK;
}

extern "C" int bn_rs_eq_eval(int n, const uint32_t* r_high, const uint32_t* rho, const uint32_t* r2, uint32_t* out) {
	BN_CHECK_ARG(n >= 0 && n <= 121, "n must be in [0, 121] (got %d)", n);
	BN_CHECK_ARG(r2 != nullptr && out != nullptr && ((r_high != nullptr && rho != nullptr) || n == 0), "NULL argument");
	// e = sum_u beta_u (x) e_u, the product over j of (1 (x) (1 ^ rho_j) + r_high,j (x) 1)
	u128p e[128], nxt[128], B[128];
	for (int u = 0; u < 128; u++) e[u] = u128p{0, 0};
	e[0] = u128p{1, 0};
	for (int j = 0; j < n; j++) {
		const u128p r = rs_elem(r_high + 4 * j);
		u128p one_rho = rs_elem(rho + 4 * j);
		one_rho.lo ^= 1;
		for (int v = 0; v < 128; v++) nxt[v] = tw_mul128_host(one_rho, e[v]);
		for (int u = 0; u < 128; u++) {
			const u128p col = tw_mul128_host(r, rs_beta(u));  // r beta_u = sum_v bit_v(col) beta_v
			for (int v = 0; v < 128; v++)
				if (rs_bit(col, v)) nxt[v] = rs_xor(nxt[v], e[u]);
		}
		for (int v = 0; v < 128; v++) e[v] = nxt[v];
	}
	rs_eq7(r2, B);
	rs_store(out, rs_dot(B, e));
	return BN_OK;
}
