// The inverse of the C++ AdditiveNTT mirror (binius-ntt_amd/host/ulvt/ntt/additive_ntt.hpp),
// built against the C-ABI alone. The reference has no inverse, so it is pinned through the
// forward transform: apply then inverse returns the input, and inverse then the oracle's forward
// returns the evaluations.
#include <cstdio>
#include <cstring>
#include <vector>

#include "finite_fields/binary_tower.hpp"
#include "ntt/additive_ntt.hpp"
#include "../../oracle/oracle.h"

static int failures = 0;
static void check(bool ok, const char* what) {
	std::printf("%s %s\n", ok ? "ok" : "FAIL", what);
	if (!ok) failures++;
}

// T = uint32_t (LIMBS 1, FanPaarTowerField<5>) or unsigned __int128 (LIMBS 4, FanPaarTowerField<7>)
template <typename T, typename P, int LIMBS>
static void round_trips(int log_h, int log_rate) {
	const size_t n = (size_t)1 << log_h;
	const char* name = LIMBS == 1 ? "u32" : "u128";
	std::vector<uint32_t> words(LIMBS * n);
	if (LIMBS == 1)
		orc_mt_fill(0xdeadbeef + log_h + log_rate, words.data(), n);
	else
		orc_fill128(0xdeadbeef + log_h + log_rate, 0x5eed0000, words.data(), n);
	AdditiveNTT<T, P> ntt(AdditiveNTTConf<T, P>(log_h, log_rate));
	NTTData<T> in(DataOrder::IN_ORDER, n), evals(n << log_rate);
	std::memcpy(in.data.get(), words.data(), in.byte_len());
	bool fwd = ntt.apply(in, evals);
	char what[128];
	for (int coset = 0; coset < (1 << log_rate); coset++) {
		// apply then inverse: block `coset` of the evaluations goes back to the input
		NTTData<T> block(DataOrder::IN_ORDER, n), back(n);
		std::memcpy(block.data.get(), evals.data.get() + (size_t)coset * n, block.byte_len());
		bool ok = fwd && ntt.inverse(block, back, coset) && back.order == DataOrder::IN_ORDER;
		ok = ok && std::memcmp(back.data.get(), words.data(), back.byte_len()) == 0;
		std::snprintf(what, sizeof(what), "AdditiveNTT<%s> log_h=%d r=%d coset=%d apply then inverse", name, log_h, log_rate, coset);
		check(ok, what);

		// inverse then the oracle's forward: arbitrary evaluations come back on block `coset`
		NTTData<T> y(DataOrder::IN_ORDER, n), x(n);
		std::vector<uint32_t> yw(LIMBS * n);
		if (LIMBS == 1)
			orc_mt_fill(0x1a7e0000 + 8 * log_h + coset, yw.data(), n);
		else
			orc_fill128(0x1a7e0000 + 8 * log_h + coset, 0x5eed0000, yw.data(), n);
		std::memcpy(y.data.get(), yw.data(), y.byte_len());
		ok = ntt.inverse(y, x, coset) && x.order == DataOrder::IN_ORDER;
		std::vector<uint32_t> want(LIMBS * (n << log_rate));
		if (LIMBS == 1)
			orc_antt32((const uint32_t*)x.data.get(), want.data(), log_h, log_rate);
		else
			orc_antt128_limbwise((const uint32_t*)x.data.get(), want.data(), log_h, log_rate);
		ok = ok && std::memcmp(want.data() + (size_t)coset * n * LIMBS, yw.data(), y.byte_len()) == 0;
		std::snprintf(what, sizeof(what), "AdditiveNTT<%s> log_h=%d r=%d coset=%d inverse then oracle forward", name, log_h, log_rate, coset);
		check(ok, what);
	}
}

static void inverse_rejects() {
	AdditiveNTT<uint32_t, FanPaarTowerField<5>> ntt(AdditiveNTTConf<uint32_t, FanPaarTowerField<5>>(4, 1));
	NTTData<uint32_t> wrong_size(DataOrder::IN_ORDER, 8), bitrev(DataOrder::BIT_REVERSED, 16), good(DataOrder::IN_ORDER, 16);
	NTTData<uint32_t> out(16), small(8);
	out.data[0] = 0x1234;
	small.data[0] = 0x5678;
	check(!ntt.inverse(wrong_size, out, 1) && !ntt.inverse(bitrev, out, 1) && out.data[0] == 0x1234 && out.order == DataOrder::INVALID,
		  "inverse returns false with no effect on bad size / order");
	check(!ntt.inverse(good, small, 1) && small.data[0] == 0x5678 && small.order == DataOrder::INVALID,
		  "inverse returns false with no effect on a short output");
	bool threw = false;
	try {
		ntt.inverse(good, out, 2);
	} catch (const std::exception&) {
		threw = true;
	}
	check(threw && out.data[0] == 0x1234, "inverse rejects a coset outside [0, 2^log_rate)");
	check(ntt.inverse(good, out, 1) && out.order == DataOrder::IN_ORDER, "inverse works after the rejected calls");
}

int main() {
	for (int log_h : {10, 13}) {
		round_trips<uint32_t, FanPaarTowerField<5>, 1>(log_h, 1);
		round_trips<unsigned __int128, FanPaarTowerField<7>, 4>(log_h, 1);
	}
	inverse_rejects();
	std::printf("%s (%d failures)\n", failures ? "FAILED" : "PASSED", failures);
	return failures ? 1 : 0;
}
