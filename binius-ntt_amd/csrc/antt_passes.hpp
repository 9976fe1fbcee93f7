// Pass planning of the bitsliced additive NTT (host only, antt_passes.cpp): tile constants, the pass
// tables the kernels take as arguments, and the planner that builds them from the subspace table.
// Tiles of 128 bitsliced 32-element blocks, host-tabulated twiddle contributions. No HIP header: the
// planner is integer code, and the device side (antt_bs_dev.hpp) includes this file for the tables.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace bn {

constexpr int kBlkBits = 7;
constexpr int kTileBlocks = 1 << kBlkBits;
constexpr int kLimbStride = 36;  // LDS words per (block, limb): 32 + 4 pad (bank spread)
constexpr int kMinLogH = kBlkBits + 5;
constexpr int kMaxStages = kBlkBits + 5;  // stages per pass
constexpr int kMaxOuter = 32 - 5 - kBlkBits;
constexpr int kMaxRateBits = 8;

enum { ROLE_FIRST = 0, ROLE_MID = 1, ROLE_LAST = 2, ROLE_SINGLE = 3 };

// bit masks of the bit-lanes p with bit j of p set (constexpr: callable from device code as it is)
constexpr uint32_t lane_mask(int j) {
	return j == 0 ? 0xAAAAAAAAu : j == 1 ? 0xCCCCCCCCu : j == 2 ? 0xF0F0F0F0u : j == 3 ? 0xFF00FF00u : 0xFFFF0000u;
}

// One pass = k consecutive stages lo..lo+k-1 over every tile. Passed by value as a kernel
// argument (~2.6 KB), so every table read is a scalar load from the kernarg segment.
struct BsPass {
	int lo, k, role, n_outer;
	int bb[kBlkBits];                        // index bit of tile block bit m
	int ob[kMaxOuter];                       // fixed (outer) index bits, ascending
	int stage_m[kMaxStages];                 // tile bit of stage lo + j (stages >= 5)
	int field[kMaxStages];                   // 8/16/32: sub-field holding every twiddle of the stage
	uint32_t twt[kMaxStages][kBlkBits];      // twiddle contribution of tile block bit m
	uint32_t two[kMaxStages][kMaxOuter];     // ... of outer bit m
	uint32_t twc[kMaxStages][kMaxRateBits];  // ... of coset bit c
	uint32_t pat[5][32];                     // stages 0..4: bit-lane part of the twiddle words
	// the same for antt_bs_pass's packed in-word stages (bottom pass): at stage s bit-lane bits
	// s..3 are index bits s+1..4 and bit-lane bit 4 is the tile's top block bit
	uint32_t pat2[5][32];
};

// Register-tile pass table (variant 4): wave w owns limb plane w of the tile; lane L holds two
// blocks R0, R1; the 7 tile bits are the register index plus six lane coordinates
//   c0 = L0^L2, c1 = L1^L2, c2 = L2, c3 = L3, c4 = L4, c5 = L5
// (partner lanes L ^ 1, 2, 7, 8, 16, 32). Before the stage on tile bit m < 6 the register bit is
// exchanged with coordinate m, so every butterfly is lane-private.
struct RtPass {
	int lo, k, role, n_outer, mlow;
	int bb[kBlkBits];
	int ob[kMaxOuter];
	int jm[kBlkBits];       // stage index (s - lo) of the block stage on tile bit m, -1 if none
	int field_m[kBlkBits];  // its class: 0 (every twiddle zero), 2, 4 or the pass table's 8 / 16 / 32
	int field_s[5];         // in-word stages s = 0..4 (bottom pass)
	uint32_t tau[kBlkBits][6];  // block stage on tile bit m: twiddle contribution of lane bit b
	uint32_t tau_iw[5][6];      // in-word stage s: lane-bit contributions to block R1's twiddle
	uint32_t cb_const[5];       // in-word stage s: R1's tile-bit-0 contribution
	uint32_t two[kMaxStages][kMaxOuter];
	uint32_t twc[kMaxStages][kMaxRateBits];
	uint32_t pat[5][32];  // in-word stage s: bit-lane part of the twiddle words (R0/R1 difference folded)
};

// precompute_subspace_evals (src/ulvt/ntt/additive_ntt.cuh:273-309), GF(2^32) values: log_h rows of
// width = log_h + log_rate - 1 columns, row-major.
void subspace_evals(int log_h, int log_rate, std::vector<uint32_t>& s);

// the sizes the bitsliced passes are built for
bool bs_supports(int log_h, int log_rate);
// largest stage field of a pass (8, 16 or 32): selects its kernel instance
int pass_fmax(const BsPass& p);

// Everything a plan needs of its passes, from the subspace table `s` of (log_h, log_rate): the pass
// tables in launch order (top stages first, the bottom pass last) and the register-tile table of every
// pass. BN_ERR_UNSUPPORTED (and the error text set) when the bottom pass's tile is not the contiguous
// run its kernels address, or a pass's stage bits are not the top tile bits.
int plan_pass_tables(int log_h, int log_rate, const std::vector<uint32_t>& s, std::vector<BsPass>& passes,
                     std::vector<RtPass>& rt);

}  // namespace bn
