// Host-side planning of the additive NTT: the subspace table, the split of a transform into passes,
// the pass tables of the LDS-tile kernels (BsPass, antt_bs.hip / antt_inv.hip) and of the register-tile
// kernels (RtPass, antt_rr.hip), the choice of a kernel instance per launch (ntt_plan_launch), and the
// two host-only exports that show the tables to the tests.
// Integer code on (log_h, log_rate, subspace table): no device, no plan.
#include "antt_passes.hpp"

#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "common.hpp"
#include "tower.hpp"

namespace bn {

void subspace_evals(int log_h, int log_rate, std::vector<uint32_t>& s) {
	const int width = log_h + log_rate - 1;
	s.assign((size_t)log_h * (size_t)std::max(width, 1), 0u);
	auto at = [&](int i, int j) -> uint32_t& { return s[(size_t)i * (size_t)width + (size_t)j]; };
	std::vector<uint32_t> norm((size_t)std::max(log_h, 1));
	for (int i = 1; i < log_h + log_rate; i++) at(0, i - 1) = 1u << i;
	norm[0] = 1;
	for (int i = 1; i < log_h; i++) {
		const uint64_t np = norm[i - 1];
		const uint64_t p0 = at(i - 1, 0);
		norm[i] = (uint32_t)(tw_square(p0, 5) ^ tw_mul(np, p0, 5));
		for (int j = 1; j < log_h + log_rate - i; j++) {
			const uint64_t sp = at(i - 1, j);
			at(i, j - 1) = (uint32_t)(tw_square(sp, 5) ^ tw_mul(np, sp, 5));
		}
	}
	for (int i = 0; i < log_h; i++) {
		const uint64_t inv = tw_inv(norm[i], 5);
		for (int j = 0; j < log_h + log_rate - i - 1; j++) at(i, j) = (uint32_t)tw_mul(inv, at(i, j), 5);
	}
}

bool bs_supports(int log_h, int log_rate) {
	return log_h >= kMinLogH && log_h - 5 - kBlkBits <= kMaxOuter && log_rate <= kMaxRateBits;
}

int pass_fmax(const BsPass& p) {
	int f = 8;
	for (int j = 0; j < p.k; j++) f = std::max(f, p.field[j]);
	return f;
}

static std::vector<BsPass> plan_passes(int log_h, int log_rate, const std::vector<uint32_t>& s_tab) {
	const int width = log_h + log_rate - 1;
	auto S = [&](int s, int kk) -> uint32_t {  // s[s][kk], 0 outside the table
		if (kk < 0 || kk >= width - s) return 0u;
		return s_tab[(size_t)s * width + kk];
	};
	std::vector<BsPass> passes;
	auto make = [&](int lo, int k, bool bottom) {
		BsPass p{};
		p.lo = lo;
		p.k = k;
		std::vector<int> bits;
		if (bottom) {
			for (int b = 5; b < 5 + kBlkBits; b++) bits.push_back(b);
		} else {
			// stage bits plus the lowest non-word batch bits (adjacent blocks in memory)
			for (int b = 5; (int)bits.size() < kBlkBits - k; b++) bits.push_back(b);
			for (int b = lo; b < lo + k; b++) bits.push_back(b);
		}
		for (int m = 0; m < kBlkBits; m++) p.bb[m] = bits[m];
		p.n_outer = 0;
		for (int b = 5; b < log_h; b++)
			if (std::find(bits.begin(), bits.end(), b) == bits.end()) p.ob[p.n_outer++] = b;
		for (int j = 0; j < k; j++) {
			const int s = lo + j;
			// twiddle of a butterfly block = XOR of s[s][kk] over the set bits kk of
			// (coset << (log_h-1-s)) | (index >> (s+1)); index bit b contributes s[s][b-s-1]
			uint32_t acc = 0;
			for (int kk = 0; kk < width - s; kk++) acc |= S(s, kk);
			p.field[j] = acc < 256u ? 8 : acc < 65536u ? 16 : 32;
			p.stage_m[j] = -1;
			for (int m = 0; m < kBlkBits; m++) {
				if (p.bb[m] == s) p.stage_m[j] = m;
				p.twt[j][m] = S(s, p.bb[m] - s - 1);
			}
			for (int m = 0; m < p.n_outer; m++) p.two[j][m] = S(s, p.ob[m] - s - 1);
			for (int c = 0; c < log_rate; c++) p.twc[j][c] = S(s, log_h - 1 - s + c);
			if (s < 5) {
				// bit-lane p of a word has index bits 0..4 = p: bits s+1..4 contribute per lane
				for (int i = 0; i < 32; i++) {
					uint32_t w = 0;
					for (int b = s + 1; b < 5; b++)
						if ((S(s, b - s - 1) >> i) & 1) w ^= lane_mask(b);
					// A's v-lanes sit on the u positions with twiddle cb ^ twt[s][6] (qa, qb differ in
					// tile bit 6 only): fold that uniform difference in
					if ((p.twt[j][kBlkBits - 1] >> i) & 1) w ^= ~lane_mask(s);
					p.pat[s][i] = w;
				}
				// packed in-word stages (antt_bs_pass): the stages above s have rotated index bit b
				// onto bit-lane bit b - 1, and bit-lane bit 4 is the tile's top block bit
				for (int i = 0; i < 32; i++) {
					uint32_t w = 0;
					for (int b = s + 1; b < 5; b++)
						if ((S(s, b - s - 1) >> i) & 1) w ^= lane_mask(b - 1);
					if ((p.twt[j][kBlkBits - 1] >> i) & 1) w ^= lane_mask(4);
					p.pat2[s][i] = w;
				}
			}
		}
		return p;
	};
	// the bottom pass runs all 12 stages of a tile (7 + 6 + 11 at 2^24 measured slower: DESIGN.md
	// section 5.6)
	constexpr int bottom_k = kMinLogH;
	const int rest = log_h - bottom_k;
	const int n_up = (rest + kBlkBits - 1) / kBlkBits;
	auto gf8_stage = [&](int s) {
		uint32_t acc = 0;
		for (int kk = 0; kk < width - s; kk++) acc |= S(s, kk);
		return acc < 256u;
	};
	// upper passes, executed first (highest stages first)
	int hi = log_h;
	for (int i = 0; i < n_up; i++) {
		const int remaining_up = n_up - i;
		int k = (hi - bottom_k + remaining_up - 1) / remaining_up;
		// the first pass takes every top stage whose twiddles lie in GF(2^8) (up to a tile's 7 bits,
		// as long as the later passes still fit): its register-tile kernel runs near the HBM rate with
		// VALU to spare, and each stage it takes leaves the GF(2^32) pass one stage less
		if (i == 0 && remaining_up > 1) {
			int g = 0;
			while (g < kBlkBits && hi - g - 1 >= bottom_k && gf8_stage(hi - g - 1)) g++;
			const int min_first = (hi - bottom_k) - (remaining_up - 1) * kBlkBits;  // the rest must still fit
			if (g > k && g >= min_first) k = g;
		}
		passes.push_back(make(hi - k, k, false));
		hi -= k;
	}
	passes.push_back(make(0, bottom_k, true));
	for (size_t i = 0; i < passes.size(); i++) {
		const bool first = i == 0, last = i + 1 == passes.size();
		passes[i].role = first && last ? ROLE_SINGLE : first ? ROLE_FIRST : last ? ROLE_LAST : ROLE_MID;
	}
	return passes;
}

// plan_passes gives the bottom pass the tile bits bb[m] = 5 + m; its kernels rely on it
static bool bottom_tile_contiguous(const BsPass& p) {
	for (int m = 0; m < kBlkBits; m++)
		if (p.bb[m] != 5 + m) return false;
	return true;
}

// lane bits that lane coordinate c_k depends on
static const int kCoordDeps[6][2] = {{0, 2}, {1, 2}, {2, -1}, {3, -1}, {4, -1}, {5, -1}};

// Sub-field class of stage j of a pass for the register-tile block stages: the smallest of 0 (every
// twiddle of the stage is zero), 2, 4 bits that holds every contribution of the stage (tile, outer
// and coset bits: a twiddle is an XOR of them), else the pass's own 8 / 16 / 32 (BsPass::field)
static int rt_stage_class(const BsPass& p, int j) {
	uint32_t acc = 0;
	for (int m = 0; m < kBlkBits; m++) acc |= p.twt[j][m];
	for (int m = 0; m < kMaxOuter; m++) acc |= p.two[j][m];
	for (int c = 0; c < kMaxRateBits; c++) acc |= p.twc[j][c];
	return acc == 0 ? 0 : acc < 4u ? 2 : acc < 16u ? 4 : p.field[j];
}

// register-tile table of a pass; false when the stage bits are not the top tile bits
static bool make_rt(const BsPass& p, bool bottom, RtPass* out) {
	RtPass r;
	memset(&r, 0, sizeof r);
	r.lo = p.lo;
	r.k = p.k;
	r.role = p.role;
	r.n_outer = p.n_outer;
	memcpy(r.bb, p.bb, sizeof r.bb);
	memcpy(r.ob, p.ob, sizeof r.ob);
	memcpy(r.two, p.two, sizeof r.two);
	memcpy(r.twc, p.twc, sizeof r.twc);
	for (int m = 0; m < kBlkBits; m++) r.jm[m] = -1;
	for (int j = 0; j < p.k; j++)
		if (p.stage_m[j] >= 0) {
			r.jm[p.stage_m[j]] = j;
			r.field_m[p.stage_m[j]] = rt_stage_class(p, j);
		}
	r.mlow = kBlkBits;
	for (int m = 0; m < kBlkBits; m++)
		if (r.jm[m] >= 0) r.mlow = std::min(r.mlow, m);
	// the stage bits must be the top tile bits (stages run from tile bit 6 down)
	for (int m = r.mlow; m < kBlkBits; m++)
		if (r.jm[m] < 0) return false;
	if (bottom && r.mlow != 0) return false;
	auto add_coords = [&](uint32_t* tau, int kmin, const uint32_t* twt) {
		for (int k = kmin; k < 6; k++)
			for (int b : kCoordDeps[k])
				if (b >= 0) tau[b] ^= twt[k + 1];
	};
	for (int m = r.mlow; m < kBlkBits; m++) add_coords(r.tau[m], m, p.twt[r.jm[m]]);
	if (bottom) {
		for (int s = 0; s < 5; s++) {
			const int j = s - p.lo;
			r.field_s[s] = p.field[j];
			r.cb_const[s] = p.twt[j][0];
			add_coords(r.tau_iw[s], 0, p.twt[j]);
			for (int i = 0; i < 32; i++) {
				// p.pat folds the variant-1 block difference (tile bit 6); fold tile bit 0 instead
				uint32_t v = p.pat[s][i];
				if ((p.twt[j][kBlkBits - 1] >> i) & 1) v ^= ~lane_mask(s);
				if ((p.twt[j][0] >> i) & 1) v ^= ~lane_mask(s);
				r.pat[s][i] = v;
			}
		}
	}
	*out = r;
	return true;
}

// ob[] of a pass as at most two runs of consecutive index bits (TileStart::mask / shift); false when
// ob[] is anything else. The description is checked against ob[] bit by bit.
static bool outer_runs(const BsPass& p, TileStart* t) {
	int r0 = 0;  // length of the first run
	while (r0 < p.n_outer && p.ob[r0] == p.ob[0] + r0) r0++;
	t->n_outer = p.n_outer;
	t->mask[0] = (uint32_t)(((uint64_t)1 << r0) - 1);
	t->shift[0] = p.n_outer > 0 ? p.ob[0] : 0;
	t->mask[1] = (uint32_t)(((uint64_t)1 << p.n_outer) - 1) & ~t->mask[0];
	t->shift[1] = r0 < p.n_outer ? p.ob[r0] - r0 : 0;
	t->n_runs = p.n_outer == 0 ? 0 : r0 < p.n_outer ? 2 : 1;
	if (t->shift[0] < 0 || t->shift[1] < 0) return false;
	for (int m = 0; m < p.n_outer; m++)
		if (tile_outer_off(*t, (size_t)1 << m) != (size_t)1 << p.ob[m]) return false;
	return true;
}

int plan_tile_starts(int log_rate, const std::vector<BsPass>& passes, std::vector<TileStart>& starts, std::vector<uint32_t>& ut) {
	starts.assign(passes.size(), TileStart{});
	ut.assign(passes.size() * kPassUtWords, 0u);
	for (size_t i = 0; i < passes.size(); i++) {
		const BsPass& p = passes[i];
		TileStart& t = starts[i];
		const bool bottom = p.role == ROLE_LAST || p.role == ROLE_SINGLE;
		if (p.n_outer < 0 || p.n_outer > kMaxOuter || log_rate < 0 || log_rate > kMaxRateBits || !outer_runs(p, &t))
			BN_FAIL(BN_ERR_UNSUPPORTED, "pass %zu: the outer bits are not two runs of index bits", i);
		if (bottom && t.mask[1] != 0) BN_FAIL(BN_ERR_UNSUPPORTED, "bottom pass: the outer bits are not one run of index bits");
		t.n_bits = p.n_outer + log_rate;
		t.n_chunks = (t.n_bits + kChunkBits - 1) / kChunkBits;
		if (t.n_chunks > kMaxChunks) BN_FAIL(BN_ERR_UNSUPPORTED, "pass %zu: %d outer and coset bits need more than %d chunks", i, t.n_bits, kMaxChunks);
		t.ut_word = (uint32_t)(i * kPassUtWords);
		// bit b of x = outer | coset << n_outer contributes two[j][b] or twc[j][b - n_outer]; each row by
		// one XOR from the row without its lowest set bit
		uint32_t* tab = ut.data() + t.ut_word;
		for (int c = 0; c < t.n_chunks; c++)
			for (int v = 1; v < kChunkRows; v++) {
				const int low = __builtin_ctz((unsigned)v), b = c * kChunkBits + low;
				uint32_t* row = tab + ((size_t)c * kChunkRows + v) * kMaxStages;
				const uint32_t* rest = tab + ((size_t)c * kChunkRows + (v & (v - 1))) * kMaxStages;
				for (int j = 0; j < kMaxStages; j++) {
					const uint32_t bit = j >= p.k || b >= t.n_bits ? 0u : b < p.n_outer ? p.two[j][b] : p.twc[j][b - p.n_outer];
					row[j] = rest[j] ^ bit;
				}
			}
	}
	return BN_OK;
}

int plan_pass_tables(int log_h, int log_rate, const std::vector<uint32_t>& s, std::vector<BsPass>& passes,
                     std::vector<RtPass>& rt) {
	passes = plan_passes(log_h, log_rate, s);
	if (!bottom_tile_contiguous(passes.back())) BN_FAIL(BN_ERR_UNSUPPORTED, "bottom pass: tile block bits are not index bits 5..11");
	rt.resize(passes.size());
	for (size_t i = 0; i < passes.size(); i++) {
		const bool bottom = passes[i].role == ROLE_LAST || passes[i].role == ROLE_SINGLE;
		if (!make_rt(passes[i], bottom, &rt[i])) BN_FAIL(BN_ERR_UNSUPPORTED, "register-tile pass table: stage bits are not the top tile bits");
		// the kernels place the outer bits with two masks and shifts (TileStart): a table they cannot
		// describe fails the plan here, with the other table checks
		TileStart t{};
		if (!outer_runs(passes[i], &t) || (bottom && t.mask[1] != 0))
			BN_FAIL(BN_ERR_UNSUPPORTED, "pass %zu: the outer bits are not the runs of index bits the kernels place", i);
	}
	return BN_OK;
}

BsDevKnobs bs_dev_knobs() {
	BsDevKnobs k;
#ifdef BN_DEV
	if (const char* e = getenv("BN_DEBUG_FLAGS")) k.dbg = atoi(e) & 7;
	if (const char* e = getenv("BN_SPLIT")) k.split = atoi(e);
	if (const char* e = getenv("BN_RR_LAST")) k.rr_last = atoi(e);
	if (const char* e = getenv("BN_ANTT_VARIANT"))
		if (const int v = atoi(e); v != 0 && valid_variant(v)) k.variant = v;
	k.trace = getenv("BN_TRACE") != nullptr;
#endif
	return k;
}

NttLaunch ntt_plan_launch(int limbs, int variant, bool inverse, int role, int fmax, size_t ntiles, int num_cus,
                          const BsDevKnobs& kn) {
	// fewer tiles than two per CU run at most one wave per SIMD, and take the kernels built for that
	const bool small = ntiles < (size_t)2 * (size_t)num_cus;
	const bool bottom = role == ROLE_LAST || role == ROLE_SINGLE;
	const int f8_32 = fmax <= 8 ? 8 : 32;
	// small bottom pass on register tiles without the three-waves bound: C3 0.0800-0.0802 vs 0.0822-0.0824 ms
	const bool rr_last = variant == 5 && limbs == 4 && role == ROLE_LAST && small && kn.rr_last != 0;
	// GF(2^16/32) LDS-tile upper passes of a small launch run lane-split (two waves per SIMD instead of
	// one): upper GF(2^32) pass 0.0139 vs 0.0158 ms, bottom pass 0.0514 vs 0.0496 ms, so not the bottom
	const bool split = limbs == 4 && fmax > 8 && !bottom && (kn.split >= 0 ? kn.split != 0 : small);
	if (variant != 1 && variant != 4 && variant != 5) return {-1, ntiles, 0, 0u};
	NttInstance k;
	if (inverse)  // the forward's passes in reverse: its first pass is the inverse's last
		k = {NttFamily::InvBs, limbs, role == ROLE_FIRST ? ROLE_LAST : role == ROLE_LAST ? ROLE_FIRST : role, f8_32, 0};
	else if (variant == 4 || (variant == 5 && fmax <= 8) || rr_last)
		k = {NttFamily::Rr, limbs, role, fmax <= 8 ? 8 : fmax <= 16 ? 16 : 32, limbs == 4 && role == ROLE_LAST && small ? 1 : bottom ? 3 : 1};
	else if (split)
		k = {NttFamily::Bs3, 4, role, 0, 0};
	else
		k = {NttFamily::Bs, limbs, role, f8_32, 0};
	NttLaunch l{-1, ntiles, instance_lds_bytes(k), instance_threads(k)};
	for (int i = 0; i < kNttInstanceCount && l.instance < 0; i++) {
		const NttInstance& c = kNttInstances[i];
		if (c.family == k.family && c.limbs == k.limbs && c.role == k.role && c.fmax == k.fmax && c.occ == k.occ) l.instance = i;
	}
	return l;
}

// the tables of (log_h, log_rate) without a plan, for the host-only exports
static int host_tables(int log_h, int log_rate, std::vector<BsPass>& passes, std::vector<RtPass>& rt) {
	if (!bs_supports(log_h, log_rate)) BN_FAIL(BN_ERR_UNSUPPORTED, "the bitsliced passes need log_h >= %d", kMinLogH);
	std::vector<uint32_t> s;
	subspace_evals(log_h, log_rate, s);
	return plan_pass_tables(log_h, log_rate, s, passes, rt);
}

}  // namespace bn

using namespace bn;

// Host only (no plan, no device): the bottom pass's in-word twiddle tables, for checking them
// against an independent twiddle computation. Layout: see include/binius_ntt_amd.h.
extern "C" int bn_antt_inword_tables(int log_h, int log_rate, uint32_t* out, size_t out_words) {
	constexpr size_t kStageWords = 32 + kBlkBits + kMaxOuter + kMaxRateBits + 1;
	constexpr size_t kWords = 4 + 1 + kMaxOuter + 5 * kStageWords;
	BN_CHECK_ARG(out != nullptr, "output pointer is NULL");
	BN_CHECK_ARG(log_rate >= 0 && log_rate <= 4 && log_h + log_rate <= 32, "log_h + log_rate must be <= 32, log_rate in [0,4]");
	BN_CHECK_ARG(out_words >= kWords, "output holds %zu words, need %zu", out_words, kWords);
	std::vector<BsPass> passes;
	std::vector<RtPass> rt;
	const int rc = host_tables(log_h, log_rate, passes, rt);
	if (rc != BN_OK) return rc;
	const BsPass& p = passes.back();
	uint32_t* o = out;
	*o++ = (uint32_t)kWords;
	*o++ = (uint32_t)kBlkBits;
	*o++ = (uint32_t)kMaxOuter;
	*o++ = (uint32_t)kMaxRateBits;
	*o++ = (uint32_t)p.n_outer;
	for (int m = 0; m < kMaxOuter; m++) *o++ = (uint32_t)p.ob[m];
	for (int s = 0; s < 5; s++) {
		for (int i = 0; i < 32; i++) *o++ = p.pat2[s][i];
		for (int m = 0; m < kBlkBits; m++) *o++ = p.twt[s][m];
		for (int m = 0; m < kMaxOuter; m++) *o++ = p.two[s][m];
		for (int c = 0; c < kMaxRateBits; c++) *o++ = p.twc[s][c];
		*o++ = (uint32_t)p.field[s];
	}
	return BN_OK;
}

// Host only (no plan, no device): the sub-field class the register-tile table carries for every
// stage of the upper passes, out[s - 12] for stage s = 12 .. log_h - 1.
extern "C" int bn_antt_stage_classes(int log_h, int log_rate, int32_t* out, size_t n) {
	BN_CHECK_ARG(out != nullptr, "output pointer is NULL");
	BN_CHECK_ARG(log_rate >= 0 && log_rate <= 4 && log_h + log_rate <= 32, "log_h + log_rate must be <= 32, log_rate in [0,4]");
	std::vector<BsPass> passes;
	std::vector<RtPass> rt;
	const int rc = host_tables(log_h, log_rate, passes, rt);
	if (rc != BN_OK) return rc;
	BN_CHECK_ARG(n >= (size_t)(log_h - kMinLogH), "output holds %zu entries, need %d", n, log_h - kMinLogH);
	for (size_t i = 0; i + 1 < passes.size(); i++)
		for (int m = rt[i].mlow; m < kBlkBits; m++) out[passes[i].lo + rt[i].jm[m] - kMinLogH] = rt[i].field_m[m];
	return BN_OK;
}
