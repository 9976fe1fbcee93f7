// Sumcheck round planner (host only; see sc_rounds.hpp).
#include "sc_rounds.hpp"

#include <stdlib.h>

#include <algorithm>

namespace bn {
namespace {

using namespace quad;

constexpr size_t slot_words(int G) { return G == 4 ? kQuadWords : G == 16 ? kHexWords : kWideWords; }
// product slots + the fold's broadcast challenge (128 words) + the messages' accumulators, flag and
// last-workgroup reduction
constexpr size_t lds_bytes(int G) { return ((size_t)(kScThreads / G) * slot_words(G) + 128 + 8 * (kMaxD + 1) + 1) * sizeof(uint32_t); }
constexpr size_t kPairLdsBytes = sizeof(uint32_t) * (kScThreads / 64) * kPairWaveWords;

}  // namespace

ScKnobs sc_dev_knobs() {
	ScKnobs k;
#ifdef BN_DEV
	auto num = [](const char* name, size_t dflt) {
		const char* e = getenv(name);
		return e ? (size_t)atol(e) : dflt;
	};
	k.dbg = (int)num("BN_SC_DBG", 0);
	k.hex_max = num("BN_SC_HEX_MAX", k.hex_max);
	k.wide_max = num("BN_SC_WIDE_MAX", k.wide_max);
	k.post_max = std::min(num("BN_SC_POST_MAX", k.post_max), (size_t)kAccCopies);
	k.fold_pair = num("BN_SC_FOLD_PAIR", 1) != 0;
	k.server_max_cur = num("BN_SC_SERVER_MAX_CUR", k.server_max_cur);
	k.timing = getenv("BN_SC_TIMING") != nullptr;
#endif
	return k;
}

ScLaunch sc_plan_launch(const ScShape& s, bool fold, int skip1, const ScKnobs& k) {
	ScLaunch L{};
	// (the final evaluation is its one point: there is no point 1 to skip)
	L.items = fold ? (size_t)s.d * s.n_pairs : s.n_pairs * (size_t)(s.kmax + 1 - (s.mode == 2 ? 0 : skip1));
	L.threads = kScThreads;
	// (lane pairs take 128 items per workgroup, half of sc_fold_coal's grid: below ~1.5 workgroups per
	// CU the quad fold's wider grid wins, c4 rounds 5-6: 28.0 / 24.6 vs 22.6 / 16.3 us)
	const bool quads = s.mode == 0 && L.items > k.hex_max;
	if (fold && quads && s.n_pairs % 32 == 0 && L.items >= kPairMinItems && k.fold_pair) {
		L.kernel = ScKernel::FoldPair;
		L.G = 2;
		L.lds = kPairLdsBytes;
	} else if (fold && quads && s.n_pairs % 16 == 0) {
		L.kernel = ScKernel::FoldCoal;
		L.G = 4;
	} else if (fold) {
		// one product each: the 64-lane product's extra combine phase cost what its shorter circuit
		// saved (c4 trace of round 4), and the 4-lane fold exists only coalesced
		L.kernel = s.mode == 0 ? ScKernel::Fold0G16 : ScKernel::Fold1G16;
		L.G = 16;
	} else if (s.mode != 0) {  // at most kMaxD + 1 items
		L.kernel = s.mode == 1 ? ScKernel::Messages1G64 : ScKernel::Messages2G64;
		L.G = 64;
	} else {
		L.G = L.items <= k.wide_max ? 64 : L.items <= k.hex_max ? 16 : 4;
		L.kernel = L.G == 64 ? ScKernel::Messages0G64 : L.G == 16 ? ScKernel::Messages0G16 : ScKernel::Messages0G4;
	}
	if (!L.lds) L.lds = lds_bytes(L.G);
	L.per_wg = (size_t)kScThreads / L.G;
	L.grid = (L.items + L.per_wg - 1) / L.per_wg;
	L.post = L.grid <= k.post_max;
	L.post_kernel = !fold && !L.post;
	return L;
}

size_t sc_max_lds_bytes() { return std::max({lds_bytes(4), lds_bytes(16), lds_bytes(64), kPairLdsBytes}); }

size_t srv_lds_bytes() { return ((size_t)kSrvGroups * kWideWords + 128 + 4 * (kMaxD + 1) + 6) * sizeof(uint32_t); }

}  // namespace bn
