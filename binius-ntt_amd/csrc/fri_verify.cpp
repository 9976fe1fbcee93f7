// The verifier's side of the FRI-Binius fold (host only: no plan, no device): what the 2^arity
// elements of one opened leaf fold to, by the per-pair rule of antt_fold.hip with the twiddles taken
// from the subspace table of (log_h, log_rate) at the leaf's global pair indices.
#include <string.h>

#include <vector>

#include "antt_passes.hpp"
#include "common.hpp"
#include "tower.hpp"

namespace bn {

constexpr int kLeafMaxArity = 8;  // antt_fold.hip's kFoldMaxArity

// The subspace table of the calling thread's last (log_h, log_rate): a verifier folds every query
// of a proof against one table.
static const std::vector<uint32_t>& leaf_subspace_table(int log_h, int log_rate) {
	thread_local int have_h = -1, have_rate = -1;
	thread_local std::vector<uint32_t> s;
	if (have_h != log_h || have_rate != log_rate) {
		subspace_evals(log_h, log_rate, s);
		have_h = log_h;
		have_rate = log_rate;
	}
	return s;
}

static u128p leaf_elem(const uint32_t* w) { return u128p{w[0] | ((uint64_t)w[1] << 32), w[2] | ((uint64_t)w[3] << 32)}; }

// t * a, limb by limb in GF(2^32)
static u128p leaf_mul32(uint32_t t, u128p a) {
	const uint8_t* tab = tw_mul8_table();
	auto limb = [&](uint64_t x) { return tw_mul_h<5>(tab, t, x & 0xffffffffu); };
	return u128p{limb(a.lo) | (limb(a.lo >> 32) << 32), limb(a.hi) | (limb(a.hi >> 32) << 32)};
}

}  // namespace bn

using namespace bn;

extern "C" int bn_antt_fri_fold_leaf(int log_h, int log_rate, int round, int arity, uint64_t index, const uint32_t* leaf,
                                     const uint32_t* challenges, uint32_t* out) {
	BN_CHECK_ARG(leaf != nullptr && challenges != nullptr && out != nullptr, "NULL argument");
	BN_CHECK_ARG(log_h >= 1 && log_rate >= 0 && log_rate <= 4 && log_h + log_rate <= 32,
	             "need 1 <= log_h, 0 <= log_rate <= 4, log_h + log_rate <= 32 (got %d, %d)", log_h, log_rate);
	BN_CHECK_ARG(round >= 0, "round must be >= 0 (got %d)", round);
	BN_CHECK_ARG(arity >= 1 && arity <= kLeafMaxArity, "arity must be in [1, %d] (got %d)", kLeafMaxArity, arity);
	BN_CHECK_ARG(round <= log_h && arity <= log_h - round, "round + arity must be <= log_h = %d (got %d + %d)", log_h, round, arity);
	const int log_out = log_h + log_rate - round - arity;
	BN_CHECK_ARG(index < ((uint64_t)1 << log_out), "index %llu is not below 2^%d", (unsigned long long)index, log_out);

	const std::vector<uint32_t>& s = leaf_subspace_table(log_h, log_rate);
	const int width = log_h + log_rate - 1;
	u128p cur[1 << kLeafMaxArity];
	for (int e = 0; e < (1 << arity); e++) cur[e] = leaf_elem(leaf + 4 * e);
	for (int l = 0; l < arity; l++) {
		const int stage = round + l, nbits = width - stage;
		const uint32_t* srow = s.data() + (size_t)stage * width;
		const u128p r = leaf_elem(challenges + 4 * l);
		for (int p = 0; p < (1 << (arity - 1 - l)); p++) {
			const uint64_t pair = (index << (arity - 1 - l)) | (uint64_t)p;  // the global pair index of this level
			uint32_t t = 0;
			for (int b = 0; b < nbits; b++) t ^= ((pair >> b) & 1) ? srow[b] : 0u;
			u128p u = cur[2 * p], v = cur[2 * p + 1];
			v.lo ^= u.lo;
			v.hi ^= u.hi;
			const u128p tv = leaf_mul32(t, v);
			u.lo ^= tv.lo;
			u.hi ^= tv.hi;
			const u128p rd = tw_mul128_host(r, u128p{u.lo ^ v.lo, u.hi ^ v.hi});
			cur[p] = u128p{u.lo ^ rd.lo, u.hi ^ rd.hi};
		}
	}
	out[0] = (uint32_t)cur[0].lo;
	out[1] = (uint32_t)(cur[0].lo >> 32);
	out[2] = (uint32_t)cur[0].hi;
	out[3] = (uint32_t)(cur[0].hi >> 32);
	return BN_OK;
}
