// Host-only sweep of the eq-indicator expansion's pass planner (binius-ntt_amd/csrc/eq_plan.cpp) and
// of the address functions the kernel uses (eq_plan.hpp), compiled with AddressSanitizer and UBSan
// by tests/test_eq_plan_host.py. No library, no GPU. For every (num_vars, cap):
//   - the levels sum to num_vars, each in [1, cap], the last min(num_vars, cap), shifts consistent;
//   - every pass's results partition [0, 2^n) at its stride 2^S (enumerated up to 2^16 results a
//     pass, by the tiles' end points above that);
//   - a tile's head is its own result 0, inside its range, and is a result of the pass before;
//   - the 64-bit indices do not wrap where a 32-bit shift would (n = 30).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "eq_plan.hpp"

using namespace bn;

static int failures = 0;
#define CHECK(cond, ...)                  \
	do {                                  \
		if (!(cond)) {                    \
			std::printf("FAIL ");         \
			std::printf(__VA_ARGS__);     \
			std::printf("\n");            \
			failures++;                   \
		}                                 \
	} while (0)

static void sweep(int n, int max_levels) {
	const int cap = max_levels ? max_levels : kEqTileLevels;
	EqPlan pl;
	CHECK(eq_plan(n, max_levels, &pl), "eq_plan(%d, %d) rejected", n, max_levels);
	CHECK(pl.n_passes == (n + cap - 1) / cap && pl.n_passes <= kEqMaxPasses, "n=%d cap=%d: %d passes", n, cap, pl.n_passes);
	int sum = 0;
	for (int p = 0; p < pl.n_passes; p++) {
		const EqPass& ps = pl.pass[p];
		CHECK(ps.levels >= 1 && ps.levels <= cap, "n=%d cap=%d pass %d: %d levels", n, cap, p, ps.levels);
		CHECK(p == 0 || ps.levels == cap, "n=%d cap=%d pass %d: only the first pass may be short", n, cap, p);
		sum += ps.levels;
		CHECK(ps.shift == n - sum, "n=%d cap=%d pass %d: shift %d, %d levels to come", n, cap, p, ps.shift, n - sum);
		CHECK(eq_lds_bytes(ps.levels) <= kEqLdsPerCu, "n=%d cap=%d pass %d: LDS", n, cap, p);
	}
	CHECK(sum == n, "n=%d cap=%d: levels sum to %d", n, cap, sum);
	if (pl.n_passes) CHECK(pl.pass[pl.n_passes - 1].levels == (n < cap ? n : cap), "n=%d cap=%d: last pass", n, cap);

	const uint64_t N = (uint64_t)1 << n;
	for (int p = 0; p < pl.n_passes; p++) {
		const EqPass& ps = pl.pass[p];
		const uint64_t tiles = eq_tiles(n, ps), per = (uint64_t)1 << ps.levels, stride = (uint64_t)1 << ps.shift;
		CHECK(p != 0 || tiles == 1, "n=%d cap=%d: the first pass has %llu tiles", n, cap, (unsigned long long)tiles);
		CHECK(tiles * per * stride == N, "n=%d cap=%d pass %d: results x stride != 2^n", n, cap, p);
		CHECK(eq_grid(tiles, ps.levels, 256) >= 1 && eq_grid(tiles, ps.levels, 256) <= tiles && eq_grid(tiles, ps.levels, 256) <= 512,
		      "n=%d cap=%d pass %d: grid", n, cap, p);
		// the tiles' end points, every tile up to 2^12 of them and the last ones beyond
		for (uint64_t t = 0; t < tiles; t = (t == 4095 && tiles > 8192 ? tiles - 4096 : t + 1)) {
			const uint64_t lo = eq_out_index(ps, t, 0), hi = eq_out_index(ps, t, per - 1);
			// written out in 128 bits: what the 64-bit functions must equal
			const unsigned __int128 wlo = ((unsigned __int128)t << ps.levels) << ps.shift;
			const unsigned __int128 whi = (((unsigned __int128)t << ps.levels) | (per - 1)) << ps.shift;
			CHECK(lo == wlo && hi == whi, "n=%d cap=%d pass %d tile %llu: index wrapped", n, cap, p, (unsigned long long)t);
			CHECK(lo == t * per * stride && hi == lo + (per - 1) * stride && hi < N, "n=%d cap=%d pass %d tile %llu: range", n, cap, p,
			      (unsigned long long)t);
			const uint64_t head = eq_head_index(ps, t);
			CHECK(head == lo && head >= lo && head <= hi, "n=%d cap=%d pass %d tile %llu: head outside its range", n, cap, p,
			      (unsigned long long)t);
			if (p > 0) {  // the head was written by the pass before: its tile t >> L', result t & (2^L' - 1)
				const EqPass& pr = pl.pass[p - 1];
				const uint64_t pm = ((uint64_t)1 << pr.levels) - 1;
				CHECK(eq_out_index(pr, t >> pr.levels, t & pm) == head, "n=%d cap=%d pass %d tile %llu: head not a result of pass %d", n,
				      cap, p, (unsigned long long)t, p - 1);
				CHECK((t >> pr.levels) < eq_tiles(n, pr), "n=%d cap=%d pass %d tile %llu: no such tile before", n, cap, p,
				      (unsigned long long)t);
			}
		}
		// enumerated: every multiple of the stride exactly once, nothing else
		if (tiles * per <= (1u << 16)) {
			std::vector<uint8_t> hit(tiles * per, 0);
			for (uint64_t t = 0; t < tiles; t++)
				for (uint64_t z = 0; z < per; z++) {
					const uint64_t i = eq_out_index(ps, t, z);
					CHECK(i % stride == 0 && i / stride < hit.size(), "n=%d cap=%d pass %d: result off the stride", n, cap, p);
					if (i % stride == 0 && i / stride < hit.size()) hit[i / stride]++;
				}
			for (size_t i = 0; i < hit.size(); i++) CHECK(hit[i] == 1, "n=%d cap=%d pass %d: slot %zu written %d times", n, cap, p, i, hit[i]);
		}
	}
	if (n == 30 && pl.n_passes) {
		const EqPass& last = pl.pass[pl.n_passes - 1];
		const uint64_t t = eq_tiles(n, last) - 1;
		CHECK(eq_out_index(last, t, ((uint64_t)1 << last.levels) - 1) == N - 1, "n=30: the last result is not element 2^30 - 1");
		// 16-byte elements: the last tile's byte offset needs 34 bits, which is why the indices are 64-bit
		CHECK((eq_out_index(last, t, 0) * 16) >> 32 == 3, "n=30: byte offset of the last tile");
	}
}

int main() {
	EqPlan pl;
	for (int n = 0; n <= kEqMaxVars; n++) {
		sweep(n, 0);
		for (int ml = kEqRegLevels; ml <= kEqTileLevels; ml++) sweep(n, ml);
	}
	CHECK(!eq_plan(-1, 0, &pl) && !eq_plan(kEqMaxVars + 1, 0, &pl), "num_vars out of range accepted");
	CHECK(!eq_plan(8, kEqRegLevels - 1, &pl) && !eq_plan(8, kEqTileLevels + 1, &pl) && !eq_plan(8, -1, &pl), "cap out of range accepted");
	CHECK(!eq_plan(8, 0, nullptr), "NULL plan accepted");
	CHECK(eq_plan(30, 0, &pl) && pl.n_passes == 3 && pl.pass[0].levels == 6 && pl.pass[1].levels == 12 && pl.pass[2].levels == 12,
	      "30 at 12 is 6 + 12 + 12");
	CHECK(eq_plan(0, 0, &pl) && pl.n_passes == 0, "no pass for num_vars == 0");
	std::printf("%s (%d failures)\n", failures ? "FAILED" : "PASSED", failures);
	return failures ? 1 : 0;
}
