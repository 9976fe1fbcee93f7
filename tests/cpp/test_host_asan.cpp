// Host-side sanitizer run (CPU, no GPU needed): built with AddressSanitizer + UBSan by
// tests/cpp/Makefile (`make -C tests/cpp asan`) together with an ASan build of the library's host
// code (binius-ntt_amd/lib-asan, hipcc -Xarch_host -fsanitize=address) and the oracle's C sources.
// It exercises
//   * the oracle (test infrastructure): tower arithmetic, every NTT form, bitslicing, the sumcheck
//     protocol, BabyBear and QM31 — and cross-checks the forms against each other;
//   * the C++ host mirror's host-only classes (FanPaarTowerField<H>, BitsliceUtils<W>, NTTData,
//     AdditiveNTTConf, BB31, QM31/interpolate_at) against the oracle;
//   * the library's host-side code: the generated bitsliced circuits behind multiply_unrolled<H>,
//     the packed-subfield helpers, bn_sumcheck_interpolate, the sumcheck round planner
//     (csrc/sc_rounds.cpp) over every round shape, the additive NTT's launch planner
//     (csrc/antt_passes.cpp) over every plan, variant and direction, the BabyBear NTT's planner
//     (csrc/bb31_plan.cpp) over every log_n with its tables interpreted on the host, the buffer checks
//     (csrc/buf_check.hpp), and the argument-checking / error paths of the C-ABI, the staged host
//     calls among them (no device present here: they must fail cleanly with a status code and leak
//     nothing);
//   * all 14 generated circuits of csrc/bitsliced_gen.hpp, compiled into this program, through
//     the conformance routine of circuit_conformance.hpp with a small trial count: every alias
//     mode, every operand in a heap allocation of exactly its documented size, so a gate that
//     indexes past an operand (the 8 shared words of bsm3x4_mul_acc's b, say) is a report.
// Prints "ok <what>" / "FAIL <what>" per check, and "md5 ..." lines that tests/test_asan.py compares
// with the reference's golden tables; exit status 0 iff every check passed (a sanitizer report
// aborts the run with a non-zero status).
#include <array>
#include <cstdio>
#include <cstring>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "finite_fields/baby_bear.hpp"
#include "finite_fields/binary_tower.hpp"
#include "finite_fields/binary_tower_simd.hpp"
#include "finite_fields/circuit_generator/unrolled/binary_tower_unrolled.hpp"
#include "ntt/nttconf.hpp"
#include "prime_field_sumcheck/interpolate.hpp"
#include "utils/bitslicing.hpp"
#include "utils/common.hpp"
#include "../../oracle/oracle.h"
#include "antt_passes.hpp"
#include "bb31_plan.hpp"
#include "buf_check.hpp"
#include "circuit_conformance.hpp"
#include "sc_rounds.hpp"

static int failures = 0;
static void check(bool ok, const char* what) {
	std::printf("%s %s\n", ok ? "ok" : "FAIL", what);
	if (!ok) failures++;
}

static std::string hex(const uint8_t* d) {
	char s[33];
	for (int i = 0; i < 16; i++) std::snprintf(s + 2 * i, 3, "%02x", d[i]);
	return s;
}

using u128 = unsigned __int128;
static u128 ld128(const uint32_t* w) {
	return (u128)w[0] | ((u128)w[1] << 32) | ((u128)w[2] << 64) | ((u128)w[3] << 96);
}

static void oracle_checks() {
	std::mt19937_64 rng(7);
	// tower: a * a^-1 == 1 at every height, 128-bit product KAT (tests.cu:172-201)
	bool ok = true;
	for (int h = 1; h <= 6; h++)
		for (int t = 0; t < 200; t++) {
			const uint64_t m = h == 6 ? ~0ull : ((1ull << (1 << h)) - 1);
			uint64_t a = rng() & m;
			if (!a) a = 1;
			ok = ok && orc_mul(a, orc_inv(a, h), h) == 1 && orc_square(a, h) == orc_mul(a, a, h);
		}
	check(ok, "oracle tower inverse / square, heights 1-6");
	const uint32_t ka[4] = {0x95323434u, 0x78593827u, 0x2755a479u, 0xf3122332u};
	const uint32_t kb[4] = {0x22048438u, 0x59347593u, 0x84794387u, 0xd3473493u};
	uint32_t kc[4];
	orc_mul128(ka, kb, kc);
	check(ld128(kc) == (((u128)0xceaa247e2dc6d28cull << 64) | 0x999c424f4b3220e5ull), "oracle GF(2^128) KAT (tests.cu:198-201)");

	// NTT: the reference MD5 input at log_h 10 (r = 0), and every GF(2^128) form against each other
	for (int log_h : {10, 12}) {
		std::vector<uint32_t> in((size_t)1 << log_h), out(in.size());
		orc_mt_fill(0xdeadbeefu + (uint32_t)log_h, in.data(), in.size());
		orc_antt32(in.data(), out.data(), log_h, 0);
		uint8_t d[16];
		orc_md5(out.data(), out.size() * 4, d);
		std::printf("md5 0 %d %s\n", log_h, hex(d).c_str());
	}
	{
		const int log_h = 9, r = 2;
		const size_t n = (size_t)1 << log_h;
		std::vector<uint32_t> x(4 * n), a(4 * (n << r)), b(a.size()), c(a.size()), e(a.size());
		orc_fill128(11, 0x5eed0000, x.data(), n);
		orc_antt128(x.data(), a.data(), log_h, r);
		orc_antt128_limbwise(x.data(), b.data(), log_h, r);
		orc_antt128_limbwise_batch(x.data(), c.data(), log_h, r, 1);
		orc_antt128_limbwise_mt(x.data(), e.data(), log_h, r, 3);
		check(a == b && b == c && c == e, "oracle GF(2^128) NTT: full, limb-wise, batched and threaded forms agree");
		std::vector<uint32_t> s32((size_t)log_h * (log_h + r - 1)), s128(4 * s32.size());
		orc_subspace_evals32(log_h, r, s32.data());
		orc_subspace_evals128(log_h, r, s128.data());
		bool same = true;
		for (size_t i = 0; i < s32.size(); i++) same = same && s128[4 * i] == s32[i] && !s128[4 * i + 1] && !s128[4 * i + 2] && !s128[4 * i + 3];
		check(same, "oracle subspace table: GF(2^32) and GF(2^128) computations agree");
	}
	{
		const int log_h = 15, batch = 3;
		std::vector<uint32_t> x(4 * ((size_t)batch << log_h)), a(x.size()), b(x.size());
		orc_fill128(5, 6, x.data(), x.size() / 4);
		orc_antt128_limbwise_batch(x.data(), a.data(), log_h, 0, batch);
		for (int i = 0; i < batch; i++)
			orc_antt128_limbwise_mt(x.data() + 4 * ((size_t)i << log_h), b.data() + 4 * ((size_t)i << log_h), log_h, 0, 8);
		check(a == b, "oracle batched NTT = per-transform threaded NTT (persistent pool, 8 threads)");
	}

	// bitslicing round trips
	{
		std::vector<uint32_t> blk(128 * 5), orig;
		for (auto& w : blk) w = (uint32_t)rng();
		orig = blk;
		orc_bitslice_many128(blk.data(), 5, 0);
		orc_bitslice_many128(blk.data(), 5, 1);
		uint32_t b32[32], o32[32];
		for (int i = 0; i < 32; i++) b32[i] = o32[i] = (uint32_t)rng();
		orc_bitslice_transpose32(b32);
		orc_bitslice_untranspose32(b32);
		check(blk == orig && std::memcmp(b32, o32, sizeof b32) == 0, "oracle bitslice round trips (128- and 32-bit)");
	}

	// sumcheck: compact and bitsliced transcripts agree, p(0) + p(1) = sum, final claim
	{
		const int n = 8, d = 3;
		std::vector<uint32_t> ev((size_t)d * 4 << n), bs(ev.size()), ch(4 * n);
		for (auto& w : ev) w = (uint32_t)rng();
		for (auto& w : ch) w = (uint32_t)rng();
		bs = ev;
		orc_bitslice_many128(bs.data(), bs.size() / 128, 0);
		std::vector<uint32_t> s1(4 * (n + 1)), p1(4 * (d + 1) * (n + 1)), s2(s1.size()), p2(p1.size());
		orc_sumcheck_run(ev.data(), n, d, 0, ch.data(), s1.data(), p1.data());
		orc_sumcheck_run(bs.data(), n, d, 1, ch.data(), s2.data(), p2.data());
		bool inv = s1 == s2 && p1 == p2;
		for (int r = 0; r < n; r++) {
			for (int i = 0; i < 4; i++) inv = inv && s1[4 * r + i] == (p1[4 * (d + 1) * r + i] ^ p1[4 * (d + 1) * r + 4 + i]);
			uint32_t nxt[4];
			orc_sumcheck_interpolate(&p1[4 * (d + 1) * r], d + 1, &ch[4 * r], nxt);
			inv = inv && std::memcmp(nxt, &s1[4 * (r + 1)], 16) == 0;
		}
		uint32_t f1[4], f2[4];
		orc_multilinear_composition(ev.data(), n, d, ch.data(), f1);
		orc_multilinear_composition_fold_mt(bs.data(), n, d, 1, ch.data(), f2, 2);
		inv = inv && std::memcmp(f1, f2, 16) == 0 && std::memcmp(f1, &s1[4 * n], 16) == 0;
		check(inv, "oracle sumcheck: compact = bitsliced transcript, protocol invariants, final claim");
	}

	// BabyBear: MD5 of the reference test input BB31(mt19937(0xdeadbeef + log_n)()) (test_ntt.cu:126-152)
	{
		const int log_n = 10;
		std::vector<uint32_t> in((size_t)1 << log_n), out(in.size());
		orc_mt_fill(0xdeadbeefu + (uint32_t)log_n, in.data(), in.size());
		orc_bb31_ntt(in.data(), out.data(), log_n, 137, 27, 0);
		uint8_t d[16];
		orc_md5(out.data(), out.size() * 4, d);
		std::printf("bb31md5 %d %s\n", log_n, hex(d).c_str());
		check(orc_bb31_mul(orc_bb31_inv(12345), 12345) == 1, "oracle BabyBear inverse");
	}
	// QM31 sumcheck on the reference test input QM31(i) (test_sumcheck.cu)
	{
		const int n = 6;
		std::vector<uint32_t> ev(2 * 4 << n), ch(4 * n), pts(12 * n);
		for (size_t i = 0; i < ev.size() / 4; i++) ev[4 * i] = (uint32_t)(i % ((1u << n)));
		for (auto& w : ch) w = (uint32_t)(rng() % 0x7fffffffu);
		orc_qm31_sumcheck_run(ev.data(), n, ch.data(), pts.data());
		check(true, "oracle QM31 sumcheck run");
	}
}

static void mirror_checks() {
	std::mt19937_64 rng(9);
	bool ok = true;
	for (int t = 0; t < 500; t++) {
		const uint32_t a = (uint32_t)rng(), b = (uint32_t)rng() | 1u;
		ok = ok && FanPaarTowerField<5>::multiply(a, b) == orc_mul32(a, b);
		ok = ok && FanPaarTowerField<5>::multiply(b, FanPaarTowerField<5>::inverse(b)) == 1u;
		ok = ok && FanPaarTowerField<3>::multiply(a & 0xff, b & 0xff) == (uint32_t)orc_mul(a & 0xff, b & 0xff, 3);
		uint32_t wa[4], wb[4], wc[4];
		for (int i = 0; i < 4; i++) wa[i] = (uint32_t)rng(), wb[i] = (uint32_t)rng();
		orc_mul128(wa, wb, wc);
		ok = ok && FanPaarTowerField<7>::multiply(ld128(wa), ld128(wb)) == ld128(wc);
		ok = ok && FanPaarTowerField<7>::multiply(ld128(wa), FanPaarTowerField<7>::inverse(ld128(wa))) == 1;
	}
	check(ok, "mirror FanPaarTowerField<3/5/7> vs oracle (multiply, inverse)");

	uint32_t blk[128], ref[128];
	for (int i = 0; i < 128; i++) blk[i] = ref[i] = (uint32_t)rng();
	BitsliceUtils<128>::bitslice_transpose(blk);
	orc_bitslice_transpose128(ref);
	bool same = std::memcmp(blk, ref, sizeof blk) == 0;
	BitsliceUtils<128>::bitslice_untranspose(blk);
	orc_bitslice_untranspose128(ref);
	same = same && std::memcmp(blk, ref, sizeof blk) == 0;
	const uint32_t val[4] = {1u, 0x80000000u, 0u, 0xffffffffu};
	BitsliceUtils<128>::repeat_value_bitsliced(blk, val);
	same = same && blk[0] == ~0u && blk[1] == 0u && blk[63] == ~0u && blk[64] == 0u && blk[127] == ~0u;
	check(same, "mirror BitsliceUtils<128> vs oracle (transpose, untranspose, repeat_value_bitsliced)");

	NTTData<u128> d(DataOrder::IN_ORDER, 16);
	check(d.byte_len() == 256 && d.order == DataOrder::IN_ORDER, "mirror NTTData");
	int thrown = 0;
	for (auto lr : std::vector<std::pair<int, int>>{{0, 0}, {30, 3}, {8, 5}, {4, -1}}) {
		try {
			AdditiveNTTConf<uint32_t, FanPaarTowerField<5>> c(lr.first, lr.second);
		} catch (const std::invalid_argument&) {
			thrown++;
		}
	}
	check(thrown == 4, "mirror AdditiveNTTConf rejects the reference's asserted cases (nttconf.cuh:55-60)");

	ok = true;
	for (int t = 0; t < 200; t++) {
		const uint32_t a = (uint32_t)rng(), b = (uint32_t)rng();
		ok = ok && (BB31(a) * BB31(b)).asUInt32() == orc_bb31_mul(a % BB31::P, b % BB31::P);
		if (a % BB31::P) ok = ok && (BB31::inv(BB31(a)) * BB31(a)) == BB31::one();
	}
	check(ok, "mirror BB31 vs oracle");

	ok = true;
	for (int t = 0; t < 50; t++) {
		uint32_t r[4], e[12], want[4];
		for (auto& w : r) w = (uint32_t)(rng() % M31::P);
		for (auto& w : e) w = (uint32_t)(rng() % M31::P);
		orc_qm31_interpolate(e, r, want);
		QM31 ev[3];
		for (int i = 0; i < 3; i++) std::memcpy(&ev[i], e + 4 * i, 16);
		QM31 rc;
		std::memcpy(&rc, r, 16);
		const QM31 got = interpolate_at(rc, ev);
		ok = ok && std::memcmp(&got, want, 16) == 0;
	}
	check(ok, "mirror QM31 interpolate_at vs oracle");
}

// The sumcheck round planner (csrc/sc_rounds.cpp, host only): every round shape the prover can
// reach, then the hand-derived selections.
static void sumcheck_planner_checks() {
	using namespace bn;
	const ScKnobs knobs;  // the product build's thresholds
	bool cover = true, pair_ok = true, coal_ok = true, post_ok = true, lds_ok = true, kernel_ok = true, small_ok = true;
	for (int k = 0; k <= 30; k++)
		for (int d = 1; d <= 8; d++)
			for (int fold = 0; fold <= 1; fold++)
				for (int skip1 = 0; skip1 <= 1; skip1++) {
					const size_t cur = (size_t)1 << k;
					if (fold && cur < 2) continue;
					const ScShape s = sc_shape(cur, d);
					const ScLaunch L = sc_plan_launch(s, fold != 0, skip1, knobs);
					cover = cover && L.grid >= 1 && (L.grid - 1) * L.per_wg < L.items && L.items <= L.grid * L.per_wg;
					if (L.kernel == ScKernel::FoldPair) pair_ok = pair_ok && s.n_pairs % 32 == 0 && L.items >= kPairMinItems;
					if (L.kernel == ScKernel::FoldCoal) coal_ok = coal_ok && s.n_pairs % 16 == 0;
					post_ok = post_ok && (L.post != 0) == (L.grid <= 64) && L.post_kernel == (!fold && !L.post);
					lds_ok = lds_ok && L.lds <= 160 * 1024 && L.lds <= sc_max_lds_bytes();
					kernel_ok = kernel_ok && (int)L.kernel >= 0 && (int)L.kernel < kScKernelCount &&
					            (fold ? L.kernel >= ScKernel::Fold0G16 : L.kernel <= ScKernel::Messages2G64);
					// the small modes have one width each, and their kernel is the mode's
					if (s.mode != 0)
						small_ok = small_ok && L.kernel == (fold ? ScKernel::Fold1G16 : s.mode == 1 ? ScKernel::Messages1G64 : ScKernel::Messages2G64);
					else
						small_ok = small_ok && L.kernel != ScKernel::Fold1G16 && L.kernel != ScKernel::Messages1G64 && L.kernel != ScKernel::Messages2G64;
				}
	check(cover, "sumcheck planner: (grid - 1) * per_wg < items <= grid * per_wg, cur 2^0..2^30 x d 1..8");
	check(pair_ok, "sumcheck planner: sc_fold_pair only with n_pairs % 32 == 0 and items >= kPairMinItems");
	check(coal_ok, "sumcheck planner: sc_fold_coal only with n_pairs % 16 == 0");
	check(post_ok, "sumcheck planner: in-kernel post exactly on grids <= 64, sc_post after the other messages");
	check(lds_ok && srv_lds_bytes() <= 160 * 1024, "sumcheck planner: dynamic LDS within 160 KiB");
	check(kernel_ok, "sumcheck planner: every selection is an instantiated kernel of its kind");
	check(small_ok, "sumcheck planner: the small modes run their own fixed-width kernels, the big mode never does");

	auto plan = [&](int log_cur, int d, bool fold, int skip1) { return sc_plan_launch(sc_shape((size_t)1 << log_cur, d), fold, skip1, knobs); };
	ScLaunch L = plan(24, 3, true, 0);
	check(L.kernel == ScKernel::FoldPair && L.grid == 6144 && L.lds == 69632, "sumcheck planner: (2^24, 3, fold) = pair, grid 6144, LDS 69632");
	L = plan(24, 3, false, 0);
	check(L.kernel == ScKernel::Messages0G4 && L.G == 4 && L.grid == 16384 && L.lds == 78628 && !L.post && L.post_kernel,
	      "sumcheck planner: (2^24, 3, messages) = <0,4>, grid 16384, LDS 78628, sc_post follows");
	L = plan(24, 3, false, 1);
	check(L.kernel == ScKernel::Messages0G4 && L.grid == 12288, "sumcheck planner: (2^24, 3, messages, skip1) = grid 12288");
	L = plan(18, 3, true, 0);
	check(L.kernel == ScKernel::FoldCoal && L.grid == 192, "sumcheck planner: (2^18, 3, fold) = coal, grid 192");
	L = plan(16, 3, true, 0);
	check(L.kernel == ScKernel::Fold0G16 && L.G == 16 && L.grid == 192, "sumcheck planner: (2^16, 3, fold) = sc_fold<0,16>, grid 192");
	L = plan(12, 3, false, 1);
	check(L.kernel == ScKernel::Messages0G64 && L.G == 64 && L.grid == 48 && L.post && !L.post_kernel,
	      "sumcheck planner: (2^12, 3, messages, skip1) = <0,64>, grid 48, in-kernel post");
	L = plan(5, 8, false, 0);
	check(L.kernel == ScKernel::Messages1G64 && L.grid == 3, "sumcheck planner: (32, 8, messages) = <1,64>, grid 3");
	L = plan(5, 8, true, 0);
	check(L.kernel == ScKernel::Fold1G16 && L.grid == 1, "sumcheck planner: (32, 8, fold) = sc_fold<1,16>, grid 1");
	bool last = true;
	for (int d = 1; d <= 8; d++) {
		L = plan(0, d, false, 0);
		last = last && L.kernel == ScKernel::Messages2G64 && L.grid == 1 && L.items == 1;
	}
	check(last, "sumcheck planner: (1, d, messages) = <2,64>, grid 1");
	// development-build overrides stay inside the instantiated set: a big-mode fold pushed off the
	// coalesced kernels runs on 16 lanes
	ScKnobs dev;
	dev.hex_max = 0;
	dev.wide_max = 0;
	L = sc_plan_launch(sc_shape(64 * 8, 3), true, 0, dev);
	check(L.kernel == ScKernel::Fold0G16, "sumcheck planner: threshold overrides choose only among instantiated kernels");
}

// The additive NTT's launch planner (csrc/antt_passes.cpp, host only): every plan the bitsliced path
// accepts, both fields, every variant, both directions, small and large launches, then the
// hand-derived selections.
static void ntt_planner_checks() {
	using namespace bn;
	constexpr int kCus = 256;
	auto is = [](const NttLaunch& l, NttFamily f, int limbs, int role, int fmax, int occ) {
		if (l.instance < 0 || l.instance >= kNttInstanceCount) return false;
		const NttInstance& k = kNttInstances[l.instance];
		return k.family == f && k.limbs == limbs && k.role == role && k.fmax == fmax && k.occ == occ;
	};
	check(kNttInstanceCount == 40, "NTT planner: the instance list has 40 entries");
	check(tile_lds_bytes(1) == 18480 && tile_lds_bytes(4) == 73920 && kSplitNT == 512 && kSplitLdsBytes == 147504 &&
	          rr::lds_bytes(1) == 9216 && rr::lds_bytes(4) == 36864,
	      "NTT planner: LDS constants (tile 18480 / 73920, lane-split 147504, register-tile staging 9216 / 36864 bytes)");
	BsDevKnobs knobs[4];  // the product build's, then BN_SPLIT=0, BN_SPLIT=1, BN_RR_LAST=0
	knobs[1].split = 0;
	knobs[2].split = 1;
	knobs[3].rr_last = 0;
	std::vector<int> hits(kNttInstanceCount, 0);
	int plans = 0;
	static bool holds[4][3][33][5];  // (role, fmax 8 / 16 / 32) occurs in the plan of (log_h, log_rate)
	bool planned = true, listed = true, geom = true, family = true;
	for (int log_h = 12; log_h <= 32; log_h++)
		for (int r = 0; r <= 4 && log_h + r <= 32; r++) {
			plans++;
			std::vector<uint32_t> s;
			std::vector<BsPass> passes;
			std::vector<RtPass> rt;
			subspace_evals(log_h, r, s);
			planned = planned && bs_supports(log_h, r) && plan_pass_tables(log_h, r, s, passes, rt) == BN_OK;
			for (const BsPass& p : passes) {
				const int fmax = pass_fmax(p), fi = fmax == 8 ? 0 : fmax == 16 ? 1 : 2;
				planned = planned && (fmax == 8 || fmax == 16 || fmax == 32) && p.role >= 0 && p.role < 4;
				holds[p.role][fi][log_h][r] = true;
				for (int limbs : {1, 4})
					for (int variant : {1, 4, 5})
						for (int inv = 0; inv <= 1; inv++) {
							// one transform (the inverse reads one coset block), then batches at two tiles per CU and above
							const size_t one = ((size_t)1 << (inv ? 0 : r)) << p.n_outer;
							const size_t large = std::max(one, (size_t)2 * kCus);
							for (size_t ntiles : {one, large, 2 * large})
								for (int kn = 0; kn < 4; kn++) {
									const NttLaunch l = ntt_plan_launch(limbs, variant, inv != 0, p.role, fmax, ntiles, kCus, knobs[kn]);
									if (l.instance < 0 || l.instance >= kNttInstanceCount) {
										listed = false;
										continue;
									}
									const NttInstance& k = kNttInstances[l.instance];
									if (kn == 0) hits[l.instance]++;
									const bool split = k.family == NttFamily::Bs3, reg = k.family == NttFamily::Rr;
									geom = geom && l.grid == ntiles && l.threads == (split ? 512u : 64u * (unsigned)limbs) && l.lds <= 160 * 1024 &&
									       l.lds == (split ? kSplitLdsBytes : reg ? rr::lds_bytes(limbs) : tile_lds_bytes(limbs));
									family = family && k.limbs == limbs && (k.family == NttFamily::InvBs) == (inv != 0) &&
									         (variant != 1 || (!reg && (limbs == 4 || !split))) && (variant != 4 || inv || reg);
								}
						}
			}
		}
	check(planned && plans == 95, "NTT planner: pass tables of log_rate 0..4 x log_h 12..32-log_rate, 95 plans");
	check(listed, "NTT planner: every selection is an entry of the instance list (product knobs, BN_SPLIT 0 / 1, BN_RR_LAST 0)");
	bool live = true;
	for (int i = 0; i < kNttInstanceCount; i++) live = live && hits[i] > 0;
	check(live, "NTT planner: every entry of the instance list is selected under the product knobs");
	check(geom, "NTT planner: workgroup size and LDS bytes are the family's constants, LDS within 160 KiB");
	check(family, "NTT planner: the instance's limbs, direction and variant are the launch's");
	// which (role, fmax) pairs a plan can hold, and a smallest plan of each: at(..) = the pair occurs at
	// (log_h, log_rate) and in no plan of a smaller log_h + log_rate (several plans can tie there)
	auto never = [&](int role, int fi) {
		for (int log_h = 12; log_h <= 32; log_h++)
			for (int r = 0; r <= 4; r++)
				if (holds[role][fi][log_h][r]) return false;
		return true;
	};
	auto at = [&](int role, int fi, int log_h, int r) {
		for (int h = 12; h <= 32; h++)
			for (int q = 0; q <= 4; q++)
				if (holds[role][fi][h][q] && h + q < log_h + r) return false;
		return holds[role][fi][log_h][r];
	};
	check(at(ROLE_FIRST, 0, 13, 0) && at(ROLE_FIRST, 1, 17, 0) && at(ROLE_FIRST, 2, 17, 4), "NTT planner: FIRST at fmax 8 / 16 / 32 from (13,0) / (17,0) / (17,4)");
	check(never(ROLE_MID, 0) && at(ROLE_MID, 1, 20, 0) && at(ROLE_MID, 2, 21, 0), "NTT planner: MID never at fmax 8, 16 / 32 from (20,0) / (21,0)");
	check(never(ROLE_LAST, 0) && at(ROLE_LAST, 1, 13, 0) && at(ROLE_LAST, 2, 17, 0), "NTT planner: LAST never at fmax 8, 16 / 32 from (13,0) / (17,0)");
	check(never(ROLE_SINGLE, 0) && at(ROLE_SINGLE, 1, 12, 0) && never(ROLE_SINGLE, 2), "NTT planner: SINGLE at fmax 16 only, (12,0)");

	// hand-derived selections, one GF(2^128) transform at rate 0 under the default variant
	auto plan_one = [&](int log_h, int variant, std::vector<BsPass>& passes) {
		std::vector<uint32_t> s;
		std::vector<RtPass> rt;
		subspace_evals(log_h, 0, s);
		std::vector<NttLaunch> ls;
		if (plan_pass_tables(log_h, 0, s, passes, rt) != BN_OK) return ls;
		for (const BsPass& p : passes) ls.push_back(ntt_plan_launch(4, variant, false, p.role, pass_fmax(p), (size_t)1 << p.n_outer, kCus, knobs[0]));
		return ls;
	};
	std::vector<BsPass> passes;
	std::vector<NttLaunch> ls = plan_one(24, 5, passes);
	check(ls.size() == 3 && is(ls[0], NttFamily::Rr, 4, ROLE_FIRST, 8, 1) && is(ls[1], NttFamily::Bs, 4, ROLE_MID, 32, 0) &&
	          is(ls[2], NttFamily::Bs, 4, ROLE_LAST, 32, 0) && ls[0].grid == 4096 && ls[2].grid == 4096,
	      "NTT planner: 2^24 = antt_rr_pass<4,0,8>, antt_bs_pass<4,1,32>, antt_bs_pass<4,2,32>, 4096 tiles each");
	ls = plan_one(20, 5, passes);
	check(ls.size() == 3 && is(ls[0], NttFamily::Rr, 4, ROLE_FIRST, 8, 1) && is(ls[1], NttFamily::Bs3, 4, ROLE_MID, 0, 0) && ls[1].threads == 512 &&
	          is(ls[2], NttFamily::Rr, 4, ROLE_LAST, 32, 1) && ls[2].grid == 256,
	      "NTT planner: one 2^20 transform = antt_rr_pass<4,0,8>, lane-split antt_bs3_pass<1>, antt_rr_pass<4,2,32,1>");
	ls = plan_one(12, 5, passes);
	check(ls.size() == 1 && pass_fmax(passes[0]) == 16 && is(ls[0], NttFamily::Bs, 4, ROLE_SINGLE, 32, 0), "NTT planner: 2^12 = SINGLE at fmax 16, antt_bs_pass<4,3,32>");
	ls = plan_one(12, 4, passes);
	check(ls.size() == 1 && is(ls[0], NttFamily::Rr, 4, ROLE_SINGLE, 16, 3), "NTT planner: 2^12 under variant 4 = antt_rr_pass<4,3,16>");
	// a batch that leaves the small launches takes the bounded bottom instance and the LDS-tile upper pass
	const NttLaunch big = ntt_plan_launch(4, 4, false, ROLE_LAST, 32, 512, kCus, knobs[0]);
	check(is(big, NttFamily::Rr, 4, ROLE_LAST, 32, 3) && is(ntt_plan_launch(4, 5, false, ROLE_LAST, 32, 512, kCus, knobs[0]), NttFamily::Bs, 4, ROLE_LAST, 32, 0) &&
	          is(ntt_plan_launch(4, 5, false, ROLE_FIRST, 32, 512, kCus, knobs[0]), NttFamily::Bs, 4, ROLE_FIRST, 32, 0),
	      "NTT planner: at two tiles per CU the bottom pass is bounded to three waves and the upper pass leaves the lane-split kernel");
	// the inverse runs the forward's passes in reverse: forward pass 0 is its compact-out top pass
	check(is(ntt_plan_launch(4, 5, true, ROLE_FIRST, 8, 4096, kCus, knobs[0]), NttFamily::InvBs, 4, ROLE_LAST, 8, 0) &&
	          is(ntt_plan_launch(1, 1, true, ROLE_LAST, 16, 16, kCus, knobs[0]), NttFamily::InvBs, 1, ROLE_FIRST, 32, 0),
	      "NTT planner: inverse roles are the forward's mirrored, fmax 16 on the GF(2^32) form");
	// development-build switches choose only among listed instances, and only where they apply
	check(is(ntt_plan_launch(4, 5, false, ROLE_MID, 32, 4096, kCus, knobs[2]), NttFamily::Bs3, 4, ROLE_MID, 0, 0) &&
	          is(ntt_plan_launch(1, 5, false, ROLE_MID, 32, 16, kCus, knobs[2]), NttFamily::Bs, 1, ROLE_MID, 32, 0) &&
	          is(ntt_plan_launch(4, 5, false, ROLE_FIRST, 32, 16, kCus, knobs[1]), NttFamily::Bs, 4, ROLE_FIRST, 32, 0) &&
	          is(ntt_plan_launch(4, 5, false, ROLE_LAST, 32, 256, kCus, knobs[3]), NttFamily::Bs, 4, ROLE_LAST, 32, 0),
	      "NTT planner: BN_SPLIT and BN_RR_LAST move a launch between listed instances");
	check(ntt_plan_launch(4, 0, false, ROLE_FIRST, 8, 16, kCus, knobs[0]).instance == -1 && ntt_plan_launch(4, 2, false, ROLE_FIRST, 8, 16, kCus, knobs[0]).instance == -1,
	      "NTT planner: variants without bitsliced passes select nothing");
	check(valid_variant(0) && valid_variant(1) && valid_variant(4) && valid_variant(5) && !valid_variant(2) && !valid_variant(3) && !valid_variant(6) && !valid_variant(-1),
	      "NTT planner: variants 0, 1, 4, 5");
}

// What the BabyBear kernels take a plan's pass tables and twiddle table to mean, as plain host code on
// canonical values: role 0 is a naive DFT down each column of each sub-problem, times the inter-pass
// twiddle w_{M_{p-1}}^(c k), in place; role 1 gathers its rows by log_pos and scatters their DFT by
// log_out; role 2 is the DFT of the whole array. Driven by the tables alone.
static std::vector<uint32_t> bb31_interpret(const bn::bb31::BbPlan& pl, const std::vector<uint32_t>& tab, const std::vector<uint32_t>& in,
                                            bool bit_reversed) {
	using namespace bn::bb31;
	const int n = pl.log_n;
	const uint32_t r_inv = orc_bb31_inv((uint32_t)(((uint64_t)1 << 32) % kP));
	auto wpow = [&](size_t e) {  // w^e out of the Montgomery-encoded table(s)
		if (!bb_hi_split(n)) return orc_bb31_mul(tab[e], r_inv);
		const uint32_t lo = tab[e & (((size_t)1 << kLoBits) - 1)], hi = tab[((size_t)1 << kLoBits) + (e >> kLoBits)];
		return orc_bb31_mul(orc_bb31_mul(lo, r_inv), orc_bb31_mul(hi, r_inv));
	};
	auto rev = [&](size_t v) {
		size_t r = 0;
		for (int i = 0; i < n; i++) r |= ((v >> i) & 1) << (n - 1 - i);
		return r;
	};
	std::vector<uint32_t> work((size_t)1 << n), out((size_t)1 << n);
	for (int pi = 0; pi < pl.n_passes; pi++) {
		BbPass p = pl.pass[pi];
		if (pi == 0) p.bitrev_in = bit_reversed;
		const size_t R = (size_t)1 << p.m;
		std::vector<uint32_t> wr(R), col(R), y(R);
		for (size_t i = 0; i < R; i++) wr[i] = wpow(i << (n - p.m));
		const uint32_t* src = pi == 0 ? in.data() : work.data();
		auto load = [&](size_t r, size_t j) { col[r] = src[p.bitrev_in ? rev(j) : j] % kP; };
		auto dft = [&]() {
			const uint32_t *x = col.data(), *w = wr.data();
			for (size_t k = 0; k < R; k++) {
				uint64_t acc = 0;
				for (size_t j = 0; j < R; j++) acc = (acc + (uint64_t)x[j] * w[(j * k) & (R - 1)]) % kP;
				y[k] = (uint32_t)acc;
			}
		};
		if (p.role == BB_SINGLE) {
			for (size_t r = 0; r < R; r++) load(r, r);
			dft();
			out = y;
		} else if (p.role == BB_UPPER) {
			for (size_t q = 0; q < (size_t)1 << (n - p.log_sub); q++)
				for (size_t c = 0; c < (size_t)1 << p.log_mp; c++) {
					for (size_t r = 0; r < R; r++) load(r, (q << p.log_sub) + (r << p.log_mp) + c);
					dft();
					for (size_t k = 0; k < R; k++)
						work[(q << p.log_sub) + (k << p.log_mp) + c] =
						    orc_bb31_mul(y[k], wpow(((c * k) & (((size_t)1 << p.log_sub) - 1)) << (n - p.log_sub)));
				}
		} else {
			for (size_t k1 = 0; k1 < (size_t)1 << p.m1; k1++)
				for (size_t g = 0; g < (size_t)1 << p.gbits; g++) {
					size_t gg = g, gpos = 0, gout = 0;
					for (int i = 0; i < p.ndig; i++) {
						const size_t d = gg & (((size_t)1 << p.mdig[i]) - 1);
						gg >>= p.mdig[i];
						gpos += d << p.log_pos[i];
						gout += d << p.log_out[i];
					}
					for (size_t r = 0; r < R; r++) load(r, (k1 << (n - p.m1)) + gpos + r);
					dft();
					for (size_t k = 0; k < R; k++) out[k1 + gout + (k << (n - p.m))] = y[k];
				}
		}
	}
	return out;
}

// The BabyBear NTT's planner (csrc/bb31_plan.cpp, host only): the digit split, the pass tables and the
// launch of every log_n, which instance each size reaches first, the twiddle table against the oracle's
// powers, and the interpreter above against the oracle's transform.
static void bb31_planner_checks() {
	using namespace bn::bb31;
	BbPlan pl;
	check(kBbInstanceCount == 9 && !bb_plan(0, &pl) && !bb_plan(kMaxLogN + 1, &pl) && kMaxLogN == 27, "BabyBear planner: 9 instances, log_n 1..27");
	check(bb_lds_bytes(BB_SINGLE, 13) == 49152 && bb_lds_bytes(BB_UPPER, 9) == 66560 && bb_lds_bytes(BB_LAST, 6) == 8320,
	      "BabyBear planner: LDS bytes (single 2^13 49152, 2^9 x 32 tile 66560, 2^6 x 32 tile 8320)");
	bool split = true, tables = true, listed = true, cover = true, lds = true;
	int first[kBbInstanceCount];
	for (int& f : first) f = 0;
	for (int log_n = 1; log_n <= kMaxLogN; log_n++) {
		split = split && bb_plan(log_n, &pl) && pl.log_n == log_n && pl.n_passes >= 1 && pl.n_passes <= kMaxPasses &&
		        (pl.n_passes == 1) == (log_n <= 13);
		if (!split) break;
		const int L = pl.n_passes;
		int used = 0;
		for (int i = 0; i < L; i++) {
			const BbPass& p = pl.pass[i];
			split = split && p.m >= 1 && (L == 1 || (p.m >= 6 && p.m <= 9));
			tables = tables && p.role == (L == 1 ? BB_SINGLE : i + 1 < L ? BB_UPPER : BB_LAST) && p.bitrev_in == 0 &&
			         p.log_sub == log_n - used && p.log_mp == p.log_sub - p.m;
			used += p.m;
			if (p.role == BB_LAST) {
				int dsum = 0;
				for (int d = 0; d < p.ndig; d++) dsum += p.mdig[d];
				tables = tables && p.m1 == pl.pass[0].m && p.ndig == L - 2 && p.gbits + p.m1 + p.m == log_n && dsum == p.gbits;
			}
			for (size_t batch : {(size_t)1, (size_t)3, (size_t)65535}) {
				const BbLaunch l = bb_plan_launch(p, log_n, batch);
				if (l.instance < 0 || l.instance >= kBbInstanceCount) {
					listed = false;
					continue;
				}
				const BbInstance& k = kBbInstances[l.instance];
				listed = listed && k.role == p.role && (p.role == BB_SINGLE ? p.m <= k.m : p.m == k.m);
				cover = cover && l.tiles * bb_tile_words(p.role, p.m) == (size_t)1 << log_n && l.batch == batch && l.threads == 256;
				lds = lds && l.lds == bb_lds_bytes(p.role, p.m) && l.lds <= bb_lds_bytes(k.role, k.m) && l.lds <= 160 * 1024;
				if (!first[l.instance]) first[l.instance] = log_n;
			}
		}
		split = split && used == log_n;
	}
	check(split, "BabyBear planner: digits sum to log_n, one pass up to 2^13, every multi-pass digit in 6..9");
	check(tables, "BabyBear planner: roles, sub-problem sizes, gbits + m1 + m_last = log_n, sum(mdig) = gbits");
	check(listed, "BabyBear planner: every launch names the listed instance of the pass's (role, m)");
	check(cover, "BabyBear planner: tiles x tile words = 2^log_n, grid y = batch, 256 threads");
	check(lds, "BabyBear planner: LDS bytes within the instance's attribute and 160 KiB");
	// the whole list is live; the smallest log_n of each entry (list order: single, role 0 m 6..9, role 1 m 6..9)
	const int want_first[kBbInstanceCount] = {1, 19, 14, 15, 17, 19, 14, 16, 18};
	check(std::memcmp(first, want_first, sizeof first) == 0,
	      "BabyBear planner: every instance is selected; first at log_n 1 (single), 14 (7s), 15 / 16 (8s), 17 / 18 (9s), 19 (6s)");

	const uint32_t mont_r = (uint32_t)(((uint64_t)1 << 32) % kP);
	for (int log_n : {10, 14}) {
		const std::vector<uint32_t> tab = bb_twiddles(137, 27, log_n);
		const uint32_t w = orc_bb31_pow(137, (uint64_t)1 << (27 - log_n));
		const size_t lo = (size_t)1 << (bb_hi_split(log_n) ? kLoBits : log_n), hi = bb_hi_split(log_n) ? (size_t)1 << (log_n - kLoBits) : 0;
		bool ok = tab.size() == lo + hi;
		for (size_t e = 0; ok && e < lo; e++) ok = tab[e] == orc_bb31_mul(orc_bb31_pow(w, e), mont_r);
		for (size_t e = 0; ok && e < hi; e++) ok = tab[lo + e] == orc_bb31_mul(orc_bb31_pow(w, e << kLoBits), mont_r);
		check(ok, log_n == 10 ? "BabyBear planner: twiddle table at 2^10 (one table) = w^e 2^32" : "BabyBear planner: twiddle table at 2^14 (lo ++ hi) = w^e 2^32");
	}
	struct Case {
		int log_n;
		bool bit_reversed;
		const char* what;
	};
	for (const Case& c : {Case{10, true, "BabyBear planner: interpreted tables = oracle at 2^10, bit-reversed (single tile)"},
	                      Case{14, false, "BabyBear planner: interpreted tables = oracle at 2^14, in order (two passes)"},
	                      Case{14, true, "BabyBear planner: interpreted tables = oracle at 2^14, bit-reversed"},
	                      Case{19, false, "BabyBear planner: interpreted tables = oracle at 2^19, in order (three passes)"}}) {
		std::vector<uint32_t> in((size_t)1 << c.log_n), want(in.size());
		orc_mt_fill(0xdeadbeefu + (uint32_t)c.log_n, in.data(), in.size());
		orc_bb31_ntt(in.data(), want.data(), c.log_n, 137, 27, c.bit_reversed);
		check(bb_plan(c.log_n, &pl) && bb31_interpret(pl, bb_twiddles(137, 27, c.log_n), in, c.bit_reversed) == want, c.what);
	}
}

static void library_host_checks() {
	std::mt19937_64 rng(11);
	check(bn_version() && std::strlen(bn_version()) > 0, "bn_version");
	// generated bitsliced circuits (host build of multiply_unrolled<H>) vs the oracle's products
	bool ok = true;
	for (int t = 0; t < 4; t++) {
		uint32_t a[128], b[128], c[128], ca[128], cb[128];
		for (int i = 0; i < 128; i++) a[i] = ca[i] = (uint32_t)rng(), b[i] = cb[i] = (uint32_t)rng();
		multiply_unrolled<7>(a, b, c);
		orc_bitslice_untranspose128(ca);
		orc_bitslice_untranspose128(cb);
		uint32_t want[128];
		for (int e = 0; e < 32; e++) orc_mul128(ca + 4 * e, cb + 4 * e, want + 4 * e);
		orc_bitslice_transpose128(want);
		ok = ok && std::memcmp(c, want, sizeof c) == 0;
		multiply_unrolled<7>(a, b, a);  // alias-safe (core.cu:21)
		ok = ok && std::memcmp(a, want, sizeof a) == 0;
		uint32_t a5[32], b5[32], c5[32];
		for (int i = 0; i < 32; i++) a5[i] = (uint32_t)rng(), b5[i] = (uint32_t)rng();
		multiply_unrolled<5>(a5, b5, c5);
		uint32_t x5[32], y5[32];
		std::memcpy(x5, a5, sizeof a5);
		std::memcpy(y5, b5, sizeof b5);
		orc_bitslice_untranspose32(x5);
		orc_bitslice_untranspose32(y5);
		uint32_t w5[32];
		for (int e = 0; e < 32; e++) w5[e] = orc_mul32(x5[e], y5[e]);
		orc_bitslice_transpose32(w5);
		ok = ok && std::memcmp(c5, w5, sizeof c5) == 0;
	}
	check(ok, "library multiply_unrolled<5>/<7> host circuits vs oracle (incl. dst == a)");

	ok = true;
	for (int t = 0; t < 100; t++) {
		const uint32_t a = (uint32_t)rng(), b = (uint32_t)rng();
		const uint32_t p = mul_binary_tower_32b_simd<3>(a, b);
		for (int l = 0; l < 4; l++)
			ok = ok && ((p >> (8 * l)) & 0xff) == (uint32_t)orc_mul((a >> (8 * l)) & 0xff, (b >> (8 * l)) & 0xff, 3);
		const auto cd = interleave_32b<2>(a, b);
		const auto back = interleave_32b<2>(cd.first, cd.second);
		ok = ok && back.first == a && back.second == b;
		(void)xor_adjacent_32b<1>(a);
	}
	check(ok, "library packed-subfield helpers (mul_binary_tower_32b_simd<3>, interleave_32b<2> involution)");

	ok = true;
	for (int npts : {2, 4, 9}) {
		std::vector<uint32_t> pts(4 * (size_t)npts);
		for (auto& w : pts) w = (uint32_t)rng();
		uint32_t r[4], got[4], want[4];
		for (auto& w : r) w = (uint32_t)rng();
		ok = ok && bn_sumcheck_interpolate(pts.data(), npts, r, got) == BN_OK;
		orc_sumcheck_interpolate(pts.data(), npts, r, want);
		ok = ok && std::memcmp(got, want, 16) == 0;
	}
	check(ok, "library bn_sumcheck_interpolate vs oracle");

	// the host-only pass planner (csrc/antt_passes.cpp) over every size it plans: log_rate 0..4 x
	// log_h 12..32 - log_rate, each output in a heap allocation of exactly the size the call asks for
	{
		uint32_t probe[512];
		check(bn_antt_inword_tables(12, 0, probe, 512) == BN_OK && probe[0] <= 512, "bn_antt_inword_tables reports its size");
		const size_t words = probe[0];
		bool tabs = true, classes = true;
		for (int log_h = 12; log_h <= 32; log_h++)
			for (int r = 0; r <= 4 && log_h + r <= 32; r++) {
				std::vector<uint32_t> t(words);
				tabs = tabs && bn_antt_inword_tables(log_h, r, t.data(), t.size()) == BN_OK && t[0] == words &&
				       (int)t[4] == log_h - 12;  // the bottom pass fixes every index bit above its tile
				for (int s = 0; s < 5 && tabs; s++) {
					const uint32_t f = t[5 + t[2] + (s + 1) * (32 + t[1] + t[2] + t[3] + 1) - 1];
					tabs = f == 8 || f == 16 || f == 32;
				}
				const size_t n = (size_t)(log_h - 12);
				std::vector<int32_t> c(n ? n : 1, -1);  // n == 0: nothing is written, the pointer must still be non-NULL
				classes = classes && bn_antt_stage_classes(log_h, r, c.data(), n) == BN_OK;
				for (size_t i = 0; i < n; i++)
					classes = classes && (c[i] == 0 || c[i] == 2 || c[i] == 4 || c[i] == 8 || c[i] == 16 || c[i] == 32);
			}
		check(tabs, "bn_antt_inword_tables, log_rate 0..4 x log_h 12..32 - log_rate");
		check(classes, "bn_antt_stage_classes, log_rate 0..4 x log_h 12..32 - log_rate");
		std::vector<uint32_t> t(words);
		std::vector<int32_t> c(4);
		check(bn_antt_inword_tables(11, 0, t.data(), t.size()) == BN_ERR_UNSUPPORTED, "bn_antt_inword_tables rejects log_h 11");
		check(bn_antt_inword_tables(12, 0, t.data(), 10) == BN_ERR_INVALID, "bn_antt_inword_tables rejects a short output");
		check(bn_antt_inword_tables(12, 5, t.data(), t.size()) == BN_ERR_INVALID, "bn_antt_inword_tables rejects log_rate 5");
		check(bn_antt_inword_tables(12, 0, nullptr, t.size()) == BN_ERR_INVALID, "bn_antt_inword_tables rejects a NULL output");
		check(bn_antt_stage_classes(11, 0, c.data(), 4) == BN_ERR_UNSUPPORTED, "bn_antt_stage_classes rejects log_h 11");
		check(bn_antt_stage_classes(16, 0, c.data(), 3) == BN_ERR_INVALID, "bn_antt_stage_classes rejects a short output");
		check(bn_antt_stage_classes(16, 5, c.data(), 4) == BN_ERR_INVALID, "bn_antt_stage_classes rejects log_rate 5");
		check(bn_antt_stage_classes(16, 0, nullptr, 4) == BN_ERR_INVALID, "bn_antt_stage_classes rejects a NULL output");
	}

	// error paths: invalid arguments are rejected before any device call; with no device the
	// device-touching calls fail with a status code (never abort), and bn_last_error says why
	bn_antt_plan* plan = reinterpret_cast<bn_antt_plan*>(&ok);
	check(bn_antt_plan_create(0, 64, 10, 0, &plan) == BN_ERR_INVALID && plan == nullptr && std::strlen(bn_last_error()) > 0,
	      "bn_antt_plan_create rejects field_bits 64");
	check(bn_antt_plan_create(0, 128, 0, 0, &plan) == BN_ERR_INVALID, "bn_antt_plan_create rejects log_h 0");
	check(bn_antt_plan_create(0, 128, 10, 5, &plan) == BN_ERR_INVALID, "bn_antt_plan_create rejects log_rate 5");
	check(bn_antt_plan_create(0, 128, 10, 0, nullptr) == BN_ERR_INVALID, "bn_antt_plan_create rejects a NULL output");
	const int rc = bn_antt_plan_create(0, 128, 10, 0, &plan);
	check(rc != BN_OK && plan == nullptr, "bn_antt_plan_create without a device fails cleanly");
	check(bn_antt_forward_device(nullptr, nullptr, nullptr, 1, nullptr) == BN_ERR_INVALID, "bn_antt_forward_device(NULL plan)");
	check(bn_antt_plan_destroy(nullptr) == BN_OK, "bn_antt_plan_destroy(NULL)");
	bn_sumcheck* sc = nullptr;
	std::vector<uint32_t> ev(4 * 8 * 3);
	check(bn_sumcheck_create(0, 3, 9, 0, ev.data(), &sc) == BN_ERR_INVALID && sc == nullptr, "bn_sumcheck_create rejects d = 9");
	check(bn_sumcheck_create(0, 3, 3, 1, ev.data(), &sc) == BN_ERR_INVALID, "bn_sumcheck_create rejects bitsliced n < 5");
	check(bn_sumcheck_interpolate(nullptr, 3, nullptr, nullptr) == BN_ERR_INVALID, "bn_sumcheck_interpolate(NULL)");
	check(bn_multiply_unrolled(8, ev.data(), ev.data(), ev.data()) == BN_ERR_INVALID, "bn_multiply_unrolled rejects height 8");
	check(bn_check_gpu_capabilities() == 0, "bn_check_gpu_capabilities without a device");
	try {
		ulvt::bn_check(bn_antt_plan_create(0, 128, 0, 0, &plan));
		check(false, "ulvt::bn_check throws BnError");
	} catch (const ulvt::BnError& e) {
		check(e.code == BN_ERR_INVALID && std::string(e.what()).find("log_h") != std::string::npos, "ulvt::bn_check throws BnError");
	}
}

// The buffer checks of the entry points (csrc/buf_check.hpp, host only), then the entry points that
// use them and the staged host calls, through the C ABI with no device present.
static void buffer_check_checks() {
	using bn::is_aligned;
	using bn::ranges_overlap;
	const auto at = [](uintptr_t a) { return reinterpret_cast<const void*>(a); };
	check(!ranges_overlap(at(0x1000), 0x100, at(0x2000), 0x100) && !ranges_overlap(at(0x2000), 0x100, at(0x1000), 0x100),
	      "ranges_overlap: disjoint ranges");
	check(!ranges_overlap(at(0x1000), 0x100, at(0x1100), 0x100) && !ranges_overlap(at(0x1100), 0x100, at(0x1000), 0x100),
	      "ranges_overlap: adjacent ranges do not overlap");
	check(ranges_overlap(at(0x1000), 0x100, at(0x10ff), 0x100) && ranges_overlap(at(0x10ff), 0x100, at(0x1000), 0x100),
	      "ranges_overlap: one shared byte");
	check(ranges_overlap(at(0x1000), 0x1000, at(0x1800), 0x10) && ranges_overlap(at(0x1800), 0x10, at(0x1000), 0x1000),
	      "ranges_overlap: nested ranges");
	check(ranges_overlap(at(0x1000), 0x100, at(0x1000), 0x100), "ranges_overlap: identical ranges");
	check(!ranges_overlap(at(0x1000), 0, at(0x1000), 0x100) && !ranges_overlap(at(0x1000), 0x100, at(0x1080), 0) &&
	          !ranges_overlap(at(0x1000), 0, at(0x1000), 0),
	      "ranges_overlap: a zero-length range overlaps nothing");
	// (the pointer form a + n <= b wrapped to 0 here and called the ranges disjoint or not by accident)
	check(!ranges_overlap(at(UINTPTR_MAX - 15), 16, at(0x1000), 0x100) && !ranges_overlap(at(0x1000), 0x100, at(UINTPTR_MAX - 15), 16) &&
	          ranges_overlap(at(UINTPTR_MAX - 15), 16, at(UINTPTR_MAX - 31), 17) && !ranges_overlap(at(UINTPTR_MAX - 15), 16, at(UINTPTR_MAX - 31), 16),
	      "ranges_overlap: a range ending at the highest address does not wrap");
	check(is_aligned(at(0x1000), 4) && is_aligned(at(0x1004), 4) && !is_aligned(at(0x1002), 4) && !is_aligned(at(0x1001), 4),
	      "is_aligned: 4 bytes");
	check(is_aligned(at(0x1000), 16) && is_aligned(at(0x1010), 16) && !is_aligned(at(0x1008), 16) && !is_aligned(at(0x100f), 16),
	      "is_aligned: 16 bytes");

	// the device entry points check their buffers before they touch the device: made-up addresses do
	alignas(16) static uint8_t mem[4096];
	uint8_t* const data = mem;          // 2^2 leaves of 2^0 elements: 64 bytes of data, 7 digests
	uint8_t* const tree = mem + 1024;
	uint32_t* const idx = reinterpret_cast<uint32_t*>(mem + 2048);
	check(bn_merkle_commit_device(data, 2, 0, data + 48, nullptr) == BN_ERR_INVALID && std::strlen(bn_last_error()) > 0,
	      "bn_merkle_commit_device rejects overlapping data and tree");
	check(bn_merkle_commit_device(data, 2, 0, tree + 8, nullptr) == BN_ERR_INVALID, "bn_merkle_commit_device rejects a misaligned tree");
	check(bn_merkle_open_device(data, tree, 2, 0, idx, 4, idx, nullptr) == BN_ERR_INVALID,
	      "bn_merkle_open_device rejects an output that overlaps the indices");
	check(bn_merkle_open_device(data, tree, 2, 0, reinterpret_cast<uint32_t*>(mem + 2050), 4, mem + 3072, nullptr) == BN_ERR_INVALID,
	      "bn_merkle_open_device rejects misaligned indices");
	uint32_t r[4 * 31] = {0}, one[4] = {0};
	check(bn_eq_expand_host(0, 31, r, nullptr, 0, one) == BN_ERR_INVALID, "bn_eq_expand_host rejects num_vars 31");
	check(bn_merkle_commit_host(0, one, 0, 9, mem) == BN_ERR_INVALID, "bn_merkle_commit_host rejects log_leaf_elems 9");
	check(bn_antt_fri_fold_host(nullptr, one, 1, 0, 1, r, one) == BN_ERR_INVALID, "bn_antt_fri_fold_host rejects a NULL plan");

	// valid staged calls with no device: a status code and a message, nothing leaked (leak detection is on)
	int rc = bn_eq_expand_host(0, 0, nullptr, nullptr, 0, one);
	check(rc != BN_OK && std::strlen(bn_last_error()) > 0, "bn_eq_expand_host without a device fails cleanly");
	uint32_t leaf[4] = {1, 2, 3, 4};
	uint8_t root[32];
	rc = bn_merkle_commit_host(0, leaf, 0, 0, root);
	check(rc != BN_OK && std::strlen(bn_last_error()) > 0, "bn_merkle_commit_host without a device fails cleanly");
}

int main() {
	oracle_checks();
	mirror_checks();
	library_host_checks();
	buffer_check_checks();
	sumcheck_planner_checks();
	ntt_planner_checks();
	bb31_planner_checks();
	failures += conformance::run_all(2);
	std::printf("%s: %d failure(s)\n", failures ? "FAILED" : "PASSED", failures);
	return failures ? 1 : 0;
}
