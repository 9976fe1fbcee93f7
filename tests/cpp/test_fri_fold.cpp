// The FRI-Binius fold of the C++ AdditiveNTT mirror (binius-ntt_amd/host/ulvt/ntt/additive_ntt.hpp),
// built against the C-ABI alone. The reference has no fold, so it is pinned by two properties: an
// arity-k fold equals k single rounds, and the codeword of x folded through all log_h rounds is
// 2^log_rate copies of the multilinear extension of x at the challenges (the oracle's
// orc_multilinear_composition, which takes the highest variable first: challenges reversed).
#include <cstdio>
#include <cstring>
#include <vector>

#include "finite_fields/binary_tower.hpp"
#include "ntt/additive_ntt.hpp"
#include "../../oracle/oracle.h"

typedef unsigned __int128 u128;
typedef FanPaarTowerField<7> F7;

static int failures = 0;
static void check(bool ok, const char* what) {
	std::printf("%s %s\n", ok ? "ok" : "FAIL", what);
	if (!ok) failures++;
}

static void folds(int log_h, int log_rate) {
	const size_t n = (size_t)1 << log_h, n_cw = n << log_rate;
	std::vector<uint32_t> words(4 * n), ch(4 * log_h);
	orc_fill128(0xdeadbeef + log_h + log_rate, 0x5eed0000, words.data(), n);
	orc_fill128(0xf01d0000 + log_h, 0xc4a11e00, ch.data(), log_h);
	AdditiveNTT<u128, F7> ntt(AdditiveNTTConf<u128, F7>(log_h, log_rate));
	NTTData<u128> in(DataOrder::IN_ORDER, n), cw(n_cw);
	std::memcpy(in.data.get(), words.data(), in.byte_len());
	const bool fwd = ntt.apply(in, cw);
	char what[128];

	// arity k at round 2 against k single rounds
	const int round = 2, k = 5;
	NTTData<u128> state(n_cw >> round);
	bool ok = fwd && ntt.fri_fold(cw, state, 0, ch.data(), round) && state.order == DataOrder::IN_ORDER;
	NTTData<u128> multi(state.size >> k);
	ok = ok && ntt.fri_fold(state, multi, round, ch.data() + 4 * round, k) && multi.order == DataOrder::IN_ORDER;
	std::vector<u128> cur(state.data.get(), state.data.get() + state.size);
	for (int i = 0; ok && i < k; i++) {
		NTTData<u128> a(DataOrder::IN_ORDER, cur.size()), b(cur.size() >> 1);
		std::memcpy(a.data.get(), cur.data(), a.byte_len());
		ok = ntt.fri_fold(a, b, round + i, ch.data() + 4 * (round + i), 1);
		cur.assign(b.data.get(), b.data.get() + b.size);
	}
	ok = ok && cur.size() == multi.size && std::memcmp(cur.data(), multi.data.get(), multi.byte_len()) == 0;
	std::snprintf(what, sizeof(what), "AdditiveNTT<u128> log_h=%d r=%d arity %d at round %d equals %d single rounds", log_h, log_rate,
	              k, round, k);
	check(ok, what);

	// the full fold, at most 8 rounds a call
	std::vector<u128> full(cw.data.get(), cw.data.get() + cw.size);
	ok = fwd;
	for (int i = 0; ok && i < log_h;) {
		const int a = log_h - i < 8 ? log_h - i : 8;
		NTTData<u128> src(DataOrder::IN_ORDER, full.size()), dst(full.size() >> a);
		std::memcpy(src.data.get(), full.data(), src.byte_len());
		ok = ntt.fri_fold(src, dst, i, ch.data() + 4 * i, a);
		full.assign(dst.data.get(), dst.data.get() + dst.size);
		i += a;
	}
	std::vector<uint32_t> rev(4 * log_h);
	for (int i = 0; i < log_h; i++) std::memcpy(rev.data() + 4 * i, ch.data() + 4 * (log_h - 1 - i), 16);
	uint32_t want[4];
	orc_multilinear_composition(words.data(), log_h, 1, rev.data(), want);
	ok = ok && full.size() == ((size_t)1 << log_rate);
	for (size_t c = 0; ok && c < full.size(); c++) ok = std::memcmp(&full[c], want, 16) == 0;
	std::snprintf(what, sizeof(what), "AdditiveNTT<u128> log_h=%d r=%d full fold is the multilinear extension", log_h, log_rate);
	check(ok, what);
}

static void fold_rejects() {
	AdditiveNTT<u128, F7> ntt(AdditiveNTTConf<u128, F7>(4, 1));
	uint32_t ch[4 * 9] = {3, 1, 4, 1, 5, 9, 2, 6};
	NTTData<u128> wrong_size(DataOrder::IN_ORDER, 16), bitrev(DataOrder::BIT_REVERSED, 32), good(DataOrder::IN_ORDER, 32);
	NTTData<u128> out(16), small(8);
	out.data[0] = 0x1234;
	small.data[0] = 0x5678;
	check(!ntt.fri_fold(wrong_size, out, 0, ch, 1) && !ntt.fri_fold(bitrev, out, 0, ch, 1) && out.data[0] == 0x1234 &&
	          out.order == DataOrder::INVALID,
	      "fri_fold returns false with no effect on bad size / order");
	check(!ntt.fri_fold(good, small, 0, ch, 1) && small.data[0] == 0x5678 && small.order == DataOrder::INVALID,
	      "fri_fold returns false with no effect on a short output");
	check(!ntt.fri_fold(good, out, 0, ch, 0) && !ntt.fri_fold(good, out, 0, ch, 5) && !ntt.fri_fold(good, out, -1, ch, 1) &&
	          !ntt.fri_fold(wrong_size, out, 1, ch, 4) && out.data[0] == 0x1234 && out.order == DataOrder::INVALID,
	      "fri_fold returns false with no effect on a bad round / arity");
	// the C-ABI's own checks
	check(bn_antt_fri_fold_host(nullptr, good.data.get(), 32, 0, 1, ch, out.data.get()) == BN_ERR_INVALID && bn_last_error()[0],
	      "bn_antt_fri_fold_host rejects a NULL plan");
	AdditiveNTT<uint32_t, FanPaarTowerField<5>> ntt32(AdditiveNTTConf<uint32_t, FanPaarTowerField<5>>(4, 1));
	NTTData<uint32_t> good32(DataOrder::IN_ORDER, 32), out32(16);
	bool threw = false;
	try {
		ntt32.fri_fold(good32, out32, 0, ch, 1);
	} catch (const std::exception&) {
		threw = true;
	}
	check(threw && out32.order == DataOrder::INVALID, "fri_fold rejects a GF(2^32) plan");
	threw = false;
	try {
		ntt.fri_fold_device(nullptr, nullptr, 0, ch, 1);
	} catch (const std::exception&) {
		threw = true;
	}
	check(threw, "fri_fold_device rejects NULL buffers");
	check(ntt.fri_fold(good, out, 0, ch, 1) && out.order == DataOrder::IN_ORDER, "fri_fold works after the rejected calls");
}

int main() {
	folds(10, 1);
	folds(13, 2);
	fold_rejects();
	std::printf("%s (%d failures)\n", failures ? "FAILED" : "PASSED", failures);
	return failures ? 1 : 0;
}
