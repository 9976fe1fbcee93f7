// The eq-indicator expansion of the C++ mirror (binius-ntt_amd/host/ulvt/sumcheck/eq_ind.hpp), built
// against the C-ABI alone. There is no reference counterpart, so it is checked against the level
// recursion (hi = A[y]*r_k, lo = A[y] ^ hi) over the oracle's orc_mul128, the sum identity (the
// elements XOR to the scale), eq_ind_eval at the expansion's own points, and the argument errors.
#include <cstdio>
#include <cstring>
#include <vector>

#include "sumcheck/eq_ind.hpp"
#include "../../oracle/oracle.h"

typedef unsigned __int128 u128;

static int failures = 0;
static void check(bool ok, const char* what) {
	std::printf("%s %s\n", ok ? "ok" : "FAIL", what);
	if (!ok) failures++;
}

static u128 mul(u128 a, u128 b) {
	u128 out;
	orc_mul128((const uint32_t*)&a, (const uint32_t*)&b, (uint32_t*)&out);
	return out;
}

static std::vector<u128> recursion(const std::vector<u128>& r, u128 scale) {
	std::vector<u128> a{scale};
	for (u128 rk : r) {
		std::vector<u128> nxt;
		nxt.reserve(2 * a.size());
		for (u128 v : a) {
			const u128 hi = mul(v, rk);
			nxt.push_back(v ^ hi);
			nxt.push_back(hi);
		}
		a.swap(nxt);
	}
	return a;
}

static void expansion(int n) {
	std::vector<u128> r(n);
	u128 scale;
	orc_fill128(0xe9e90000 + n, 0xc0ffee00, (uint32_t*)r.data(), n);
	orc_fill128(0x5ca1e000 + n, 0x5ca1e000, (uint32_t*)&scale, 1);
	char what[128];
	const std::vector<u128> want = recursion(r, scale);
	const std::vector<u128> got = eq_ind_expand(r.data(), n, scale);
	std::snprintf(what, sizeof(what), "eq_ind_expand n=%d equals the level recursion", n);
	check(got == want, what);
	const std::vector<u128> unit = eq_ind_expand(r.data(), n);
	u128 sum = 0, sum_scaled = 0;
	for (u128 v : unit) sum ^= v;
	for (u128 v : got) sum_scaled ^= v;
	std::snprintf(what, sizeof(what), "eq_ind_expand n=%d: the elements sum to the scale", n);
	check(unit.size() == ((size_t)1 << n) && sum == 1 && sum_scaled == scale, what);
	// the expansion at a boolean point is eq_ind_eval of the challenges and that point
	bool ok = true;
	for (size_t x : {(size_t)0, (size_t)1, ((size_t)1 << n) - 1, (size_t)0x1b35 & (((size_t)1 << n) - 1)}) {
		std::vector<u128> pt(n);
		for (int i = 0; i < n; i++) pt[i] = (x >> (n - 1 - i)) & 1;  // challenge i pairs with index bit n-1-i
		ok = ok && eq_ind_eval(r.data(), pt.data(), n) == unit[x] && eq_ind_eval(pt.data(), r.data(), n) == unit[x];
	}
	std::snprintf(what, sizeof(what), "eq_ind_eval n=%d at boolean points equals the expansion's elements", n);
	check(ok, what);
}

template <class F>
static bool throws_invalid(F f) {
	try {
		f();
	} catch (const ulvt::BnError& e) {
		return e.code == BN_ERR_INVALID;
	}
	return false;
}

static void rejects() {
	u128 r[4] = {3, 1, 4, 1};
	uint32_t out[4 * 16];
	check(throws_invalid([&] { eq_ind_expand(r, 31); }), "eq_ind_expand rejects 31 variables");
	check(throws_invalid([&] { eq_ind_expand(r, 4, 1, true); }), "eq_ind_expand rejects bitsliced output below one block");
	check(throws_invalid([&] { eq_ind_expand_device(r, 4, nullptr); }), "eq_ind_expand_device rejects a NULL buffer");
	check(bn_eq_expand_host(0, 4, nullptr, nullptr, 0, out) == BN_ERR_INVALID && bn_last_error()[0],
	      "bn_eq_expand_host rejects NULL challenges");
	check(throws_invalid([&] { eq_ind_eval(r, r, 129); }), "eq_ind_eval rejects 129 variables");
	const std::vector<u128> got = eq_ind_expand(r, 4);
	check(got == recursion(std::vector<u128>(r, r + 4), 1), "eq_ind_expand works after the rejected calls");
}

int main() {
	expansion(7);
	expansion(13);
	rejects();
	std::printf("%s (%d failures)\n", failures ? "FAILED" : "PASSED", failures);
	return failures ? 1 : 0;
}
