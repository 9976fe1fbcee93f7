// Pass planner of the BabyBear NTT (host only; see bb31_plan.hpp).
#include "bb31_plan.hpp"

namespace bn {
namespace bb31 {

static uint32_t h_mul(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) % kP); }
static uint32_t h_pow(uint32_t x, uint64_t e) {
	uint32_t r = 1;
	while (e) {
		if (e & 1) r = h_mul(r, x);
		x = h_mul(x, x);
		e >>= 1;
	}
	return r;
}

bool bb_plan(int log_n, BbPlan* plan) {
	if (log_n < 1 || log_n > kMaxLogN || plan == nullptr) return false;
	BbPlan pl{};
	pl.log_n = log_n;
	const int L = pl.n_passes = log_n <= kMaxSingleM ? 1 : (log_n + kMaxM - 1) / kMaxM;
	int used = 0;
	for (int i = 0; i < L; i++) {
		BbPass& p = pl.pass[i];
		p.m = log_n / L + (i < log_n % L ? 1 : 0);
		p.role = L == 1 ? BB_SINGLE : i + 1 < L ? BB_UPPER : BB_LAST;
		p.log_sub = log_n - used;
		used += p.m;
		p.log_mp = log_n - used;
	}
	// the last pass's digits 2..L-1: position stride M_i = 2^(n - m_1 - ... - m_i), output stride N_1 ... N_{i-1}
	if (L > 1) {
		BbPass& p = pl.pass[L - 1];
		p.m1 = pl.pass[0].m;
		p.gbits = log_n - p.m1 - p.m;
		int out_used = p.m1;
		for (int d = 1; d + 1 < L; d++, p.ndig++) {
			p.log_pos[p.ndig] = pl.pass[d].log_mp;
			p.log_out[p.ndig] = out_used;
			p.mdig[p.ndig] = pl.pass[d].m;
			out_used += pl.pass[d].m;
		}
	}
	*plan = pl;
	return true;
}

std::vector<uint32_t> bb_twiddles(uint32_t generator, int log_group_order, int log_n) {
	const uint32_t w = h_pow(generator % kP, (uint64_t)1 << (log_group_order - log_n));
	const uint32_t R = (uint32_t)(((uint64_t)1 << 32) % kP);
	std::vector<uint32_t> tab;
	// the powers of `base` below 2^bits, times R
	auto powers = [&](uint32_t base, int bits) {
		uint32_t cur = R;
		for (size_t e = 0; e < ((size_t)1 << bits); e++) {
			tab.push_back(cur);
			cur = h_mul(cur, base);
		}
	};
	powers(w, bb_hi_split(log_n) ? kLoBits : log_n);
	if (bb_hi_split(log_n)) powers(h_pow(w, (uint64_t)1 << kLoBits), log_n - kLoBits);
	return tab;
}

BbLaunch bb_plan_launch(const BbPass& pass, int log_n, size_t batch) {
	BbLaunch l{-1, 0, batch, bb_lds_bytes(pass.role, pass.m), kThreads};
	for (int i = 0; i < kBbInstanceCount; i++) {
		const BbInstance& k = kBbInstances[i];
		if (k.role == pass.role && (k.role == BB_SINGLE ? pass.m <= k.m : pass.m == k.m)) l.instance = i;
	}
	// every pass covers the 2^log_n words of a transform once
	l.tiles = ((size_t)1 << log_n) / bb_tile_words(pass.role, pass.m);
	return l;
}

}  // namespace bb31
}  // namespace bn
