// Pass planning of the eq-indicator expansion (host only, eq_plan.cpp): how the n levels are split
// into in-place passes, where a pass's tiles read their heads and write their results, and the
// launch shape of a pass. No HIP header: this is integer code, and the device side (eq_expand.hip)
// includes this file for the constants and the address functions, so the kernel and the host-side
// sweep (tests/cpp/test_eq_plan.cpp) use the same ones.
//
// A pass p runs L_p levels with S_p levels still to come after it. Tile y of the pass (one head,
// the table over the variables of the earlier passes at y) reads its head from element
// y << (L_p + S_p) and writes result z (L_p bits) to element ((y << L_p) | z) << S_p: the head is
// result 0 of the tile, so a tile reads only a slot of its own range before it overwrites that range,
// and the heads of pass p + 1 are exactly the results of pass p.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace bn {

constexpr int kEqMaxVars = 30;
constexpr int kEqTileLevels = 12;  // T: levels of a full pass (a tile of 2^12 results, 64 KiB)
constexpr int kEqRegLevels = 3;    // a tile's highest levels, run in registers (and the smallest cap)
constexpr int kEqMaxPasses = (kEqMaxVars + kEqRegLevels - 1) / kEqRegLevels;
constexpr int kEqThreadsLog = kEqTileLevels - kEqRegLevels;  // one thread per element of the LDS stage
constexpr int kEqThreads = 1 << kEqThreadsLog;
// LDS of a pass: one nibble table of r per level (32 positions x 16 values x 16 B; eq_expand.hip
// asserts the size) and the stage, one element per thread
constexpr size_t kEqRTabBytes = 32 * 16 * 16;
constexpr size_t kEqLdsPerCu = 160 * 1024;

struct EqPass {
	int levels;  // L_p
	int shift;   // S_p: levels of the later passes
};
struct EqPlan {
	int n_passes;
	EqPass pass[kEqMaxPasses];
};

// The split of num_vars levels at a per-pass cap of max_levels (0: kEqTileLevels): the last pass
// takes min(num_vars, cap) levels, the passes before it cap each, and the first the remainder
// (30 at 12: 6 + 12 + 12). No pass for num_vars == 0. False, with *plan untouched, unless
// 0 <= num_vars <= kEqMaxVars and max_levels is 0 or in [kEqRegLevels, kEqTileLevels].
bool eq_plan(int num_vars, int max_levels, EqPlan* plan);

constexpr uint64_t eq_tiles(int num_vars, const EqPass& p) { return (uint64_t)1 << (num_vars - p.levels - p.shift); }
constexpr uint64_t eq_head_index(const EqPass& p, uint64_t tile) { return tile << (p.levels + p.shift); }
constexpr uint64_t eq_out_index(const EqPass& p, uint64_t tile, uint64_t z) { return ((tile << p.levels) | z) << p.shift; }

constexpr size_t eq_lds_bytes(int levels) { return (size_t)levels * kEqRTabBytes + (size_t)kEqThreads * 16; }
// work-groups of a pass: one per tile up to what the device holds at once (two a CU while their
// LDS fits twice); beyond that the work-groups stride over the tiles, so that the tables of r are
// built once per resident work-group
constexpr uint64_t eq_grid(uint64_t n_tiles, int levels, int num_cus) {
	const uint64_t cap = (uint64_t)(num_cus > 0 ? num_cus : 256) * (2 * eq_lds_bytes(levels) <= kEqLdsPerCu ? 2 : 1);
	return n_tiles < cap ? n_tiles : cap;
}

}  // namespace bn
