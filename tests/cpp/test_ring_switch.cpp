// Ring-switching of the C++ mirror (binius-ntt_amd/host/ulvt/sumcheck/ring_switch.hpp), built against
// the C-ABI alone. There is no reference counterpart, so the partial evaluations at log_n = 10 and the
// linear map at 4097 compact elements and 3 bitsliced blocks are checked against the definitions
// written out bit by bit, the verifier's functions against each other through the identity
// sum_w A[w] t'[w] = s_0 over the oracle's orc_mul128, and the argument errors.
#include <cstdio>
#include <cstring>
#include <vector>

#include "sumcheck/ring_switch.hpp"
#include "utils/bitslicing.hpp"
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

static std::vector<u128> sliced(std::vector<u128> v) {
	for (size_t b = 0; b < v.size() / 32; b++) BitsliceUtils<128>::bitslice_transpose((uint32_t*)(v.data() + 32 * b));
	return v;
}

static std::vector<u128> map_by_bits(const std::vector<u128>& in, const RsTable& m) {
	std::vector<u128> out(in.size(), 0);
	for (size_t w = 0; w < in.size(); w++)
		for (int u = 0; u < 128; u++)
			if ((in[w] >> u) & 1) out[w] ^= m[u];
	return out;
}

static void partial_evals_and_identity() {
	const int log_n = 10;
	const size_t n = (size_t)1 << log_n;
	std::vector<u128> tp(n), E(n);
	u128 r2[7];
	orc_fill128(0x7a570000 + log_n, 0x5eed0000, (uint32_t*)tp.data(), n);
	orc_fill128(0xe9e90000 + log_n, 0xc0ffee00, (uint32_t*)E.data(), n);
	orc_fill128(0x22220000, 0x12120000, (uint32_t*)r2, 7);
	RsTable want{};
	for (size_t w = 0; w < n; w++)
		for (int v = 0; v < 128; v++)
			if ((tp[w] >> v) & 1) want[v] ^= E[w];
	const RsTable got = rs_partial_evals(sliced(tp).data(), sliced(E).data(), log_n);
	check(got == want, "rs_partial_evals log_n=10 equals the definition bit by bit");
	// the sumcheck's identity for any column E: sum_w map(E)[w] t'[w] == rs_sumcheck_claim(s^, r'')
	const RsTable B = rs_batch_table(r2);
	const std::vector<u128> A = gf128_linear_map(E.data(), n, B);
	check(A == map_by_bits(E, B), "gf128_linear_map of 2^10 elements by the batching table equals the definition");
	u128 sum = 0;
	for (size_t w = 0; w < n; w++) sum ^= mul(A[w], tp[w]);
	check(sum == rs_sumcheck_claim(got, r2), "sum_w A[w] t'[w] equals rs_sumcheck_claim");
	// the row check is linear in s^: of beta_0 at v alone it is eq(r_low, v), and the table's entries sum to 1
	u128 total = 0;
	for (int v = 0; v < 128; v++) {
		RsTable unit{};
		unit[v] = 1;
		total ^= rs_row_check(unit, r2);
	}
	check(total == 1 && rs_row_check(RsTable{{1}}, r2) == B[0], "rs_row_check of unit vectors gives the eq table, which sums to 1");
	check(rs_eq_eval(nullptr, nullptr, 0, r2) == B[0], "rs_eq_eval of no variables is B[0]");
}

static void linear_maps() {
	RsTable m;
	orc_fill128(0x3a70000, 0x77770000, (uint32_t*)m.data(), 128);
	std::vector<u128> x(4097);
	orc_fill128(0x11ae0000, 0x5eed0000, (uint32_t*)x.data(), x.size());
	check(gf128_linear_map(x.data(), x.size(), m) == map_by_bits(x, m), "gf128_linear_map of 4097 compact elements equals the definition");
	x.resize(96);
	check(gf128_linear_map(sliced(x).data(), 3, m, true) == sliced(map_by_bits(x, m)),
	      "gf128_linear_map of 3 bitsliced blocks is the bit transpose of the compact result");
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
	u128 buf[64] = {};
	RsTable m{};
	check(throws_invalid([&] { rs_partial_evals(buf, buf, 4); }) && throws_invalid([&] { rs_partial_evals(buf, buf, 31); }) &&
	          throws_invalid([&] { rs_partial_evals(nullptr, buf, 5); }),
	      "rs_partial_evals rejects a bad log_n and a NULL column");
	check(throws_invalid([&] { rs_partial_evals_device(nullptr, buf, 5, buf); }) &&
	          throws_invalid([&] { rs_partial_evals_device(buf, buf + 32, 5, buf + 16); }),
	      "rs_partial_evals_device rejects a NULL buffer and a result inside an input");
	check(throws_invalid([&] { gf128_linear_map(buf, 0, m); }) && throws_invalid([&] { gf128_linear_map(nullptr, 4, m); }) &&
	          throws_invalid([&] { gf128_linear_map_device(buf, buf + 1, 4, m); }),
	      "gf128_linear_map rejects no elements, a NULL input and partially overlapping buffers");
	check(throws_invalid([&] { rs_eq_eval(buf, buf, 122, buf); }) && throws_invalid([&] { rs_batch_table(nullptr); }),
	      "rs_eq_eval rejects 122 variables, rs_batch_table a NULL point");
}

int main() {
	partial_evals_and_identity();
	linear_maps();
	rejects();
	std::printf("%s (%d failures)\n", failures ? "FAILED" : "PASSED", failures);
	return failures ? 1 : 0;
}
