// The bit-reversal permutation (binius-ntt_amd/host/ulvt/utils/bit_reverse.hpp) and the verifier's leaf
// fold (AdditiveNTT::fri_fold_leaf, host/ulvt/ntt/additive_ntt.hpp) of the C++ mirror, built against
// the C-ABI alone. bit_reverse at log_n = 7 and 13 against the permutation written out bit by bit,
// applied twice, and bitsliced against BitsliceUtils; fri_fold_leaf of every leaf against fri_fold at
// (log_h 12, log_rate 1, round 0, arity 4); the argument errors.
#include <cstdio>
#include <cstring>
#include <vector>

#include "finite_fields/binary_tower.hpp"
#include "ntt/additive_ntt.hpp"
#include "utils/bit_reverse.hpp"
#include "utils/bitslicing.hpp"
#include "../../oracle/oracle.h"

typedef unsigned __int128 u128;
typedef FanPaarTowerField<7> F7;

static int failures = 0;
static void check(bool ok, const char* what) {
	std::printf("%s %s\n", ok ? "ok" : "FAIL", what);
	if (!ok) failures++;
}

static size_t rev(size_t x, int bits) {
	size_t r = 0;
	for (int i = 0; i < bits; i++) r |= ((x >> i) & 1) << (bits - 1 - i);
	return r;
}

static void permutes(int log_n) {
	const size_t n = (size_t)1 << log_n;
	std::vector<u128> in(n), want(n);
	orc_fill128(0xb17e0000 + log_n, 0xb17e5eed, (uint32_t*)in.data(), n);
	for (size_t x = 0; x < n; x++) want[rev(x, log_n)] = in[x];
	char what[128];
	const std::vector<u128> got = bit_reverse(in.data(), log_n);
	std::snprintf(what, sizeof(what), "bit_reverse log_n=%d is the index permutation", log_n);
	check(got == want, what);
	std::snprintf(what, sizeof(what), "bit_reverse log_n=%d twice is the identity", log_n);
	check(bit_reverse(got.data(), log_n) == in, what);
	std::vector<u128> sliced = want;
	for (size_t b = 0; b < n / 32; b++) BitsliceUtils<128>::bitslice_transpose((uint32_t*)(sliced.data() + 32 * b));
	std::snprintf(what, sizeof(what), "bit_reverse log_n=%d bitsliced is the bit transpose of the compact result", log_n);
	check(bit_reverse(in.data(), log_n, true) == sliced, what);
}

static void leaf_folds() {
	const int log_h = 12, log_rate = 1, round = 0, arity = 4;
	const size_t n = (size_t)1 << log_h, n_cw = n << log_rate;
	std::vector<uint32_t> ch(4 * arity);
	orc_fill128(0xf01d0000 + log_h, 0xc4a11e00, ch.data(), arity);
	AdditiveNTT<u128, F7> ntt(AdditiveNTTConf<u128, F7>(log_h, log_rate));
	NTTData<u128> in(DataOrder::IN_ORDER, n), cw(n_cw), folded(n_cw >> arity);
	orc_fill128(0xdeadbeef + log_h, 0x5eed0000, (uint32_t*)in.data.get(), n);
	bool ok = ntt.apply(in, cw) && ntt.fri_fold(cw, folded, round, ch.data(), arity);
	size_t bad = 0;
	for (size_t j = 0; ok && j < folded.size; j++)
		bad += ntt.fri_fold_leaf(round, j, cw.data.get() + (j << arity), ch.data(), arity) != folded.data[j];
	check(ok && bad == 0, "fri_fold_leaf of every leaf equals fri_fold at log_h=12 r=1 round 0 arity 4");
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
	u128 buf[32] = {};
	check(throws_invalid([&] { bit_reverse(buf, -1); }) && throws_invalid([&] { bit_reverse(buf, 31); }) &&
	          throws_invalid([&] { bit_reverse(buf, 4, true); }) && throws_invalid([&] { bit_reverse(nullptr, 3); }),
	      "bit_reverse rejects a bad log_n, bitsliced below 2^5 and a NULL input");
	check(throws_invalid([&] { bit_reverse_device(nullptr, nullptr, 5); }) && throws_invalid([&] { bit_reverse_device(buf, buf, 5); }) &&
	          throws_invalid([&] { bit_reverse_device(buf, buf + 32, 5, 0); }),
	      "bit_reverse_device rejects NULL and overlapping buffers and an empty batch");
	AdditiveNTT<u128, F7> ntt(AdditiveNTTConf<u128, F7>(5, 1));
	uint32_t ch[4 * 9] = {3, 1, 4, 1, 5, 9, 2, 6};
	check(throws_invalid([&] { ntt.fri_fold_leaf(0, 16, buf, ch, 2); }) && throws_invalid([&] { ntt.fri_fold_leaf(4, 0, buf, ch, 2); }) &&
	          throws_invalid([&] { ntt.fri_fold_leaf(0, 0, buf, ch, 0); }) && throws_invalid([&] { ntt.fri_fold_leaf(0, 0, nullptr, ch, 2); }),
	      "fri_fold_leaf rejects an index, a round, an arity out of range and a NULL leaf");
}

int main() {
	permutes(7);
	permutes(13);
	leaf_folds();
	rejects();
	std::printf("%s (%d failures)\n", failures ? "FAILED" : "PASSED", failures);
	return failures ? 1 : 0;
}
