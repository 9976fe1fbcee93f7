// Pass planning of the bitsliced additive NTT (host only, antt_passes.cpp): tile and LDS constants,
// the pass tables the kernels take as arguments, the planner that builds them from the subspace
// table, the list of pass-kernel instances, and the planner that picks one of them per launch.
// Tiles of 128 bitsliced 32-element blocks, host-tabulated twiddle contributions. No HIP header: the
// planners are integer code, and the device side (antt_bs_dev.hpp) includes this file for the tables,
// the constants and the instance list.
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

// LDS image of a tile: one plane per limb, block q of limb l at l*kPlane + q*kLimbStride (stride 36
// words: 16 consecutive blocks of one plane hit 16 distinct 4-bank groups, so a wave's
// ds_read_b128 over consecutive blocks is conflict-free).
constexpr int kPlane = kTileBlocks * kLimbStride;
// LDS of a one-wave-per-limb tile kernel (antt_bs_pass, antt_inv_bs_pass): the tile + one word per
// stage and wave for the workgroup-uniform twiddle parts
constexpr size_t tile_lds_bytes(int L) { return ((size_t)L * kPlane + (size_t)L * kMaxStages) * sizeof(uint32_t); }
// the lane-split kernel (antt_bs3_pass): 8 waves, the tile double-buffered + one word per stage
constexpr int kSplitNT = 512;
constexpr size_t kSplitLdsBytes = ((size_t)8 * kPlane + (size_t)kMaxStages) * sizeof(uint32_t);
namespace rr {  // antt_rr_pass stages half a tile through LDS: compact elements or coalesced bitsliced lines
constexpr int kSlot = 36;                // LDS words per staged block (32 + 4 pad: conflict-free b128 writes)
constexpr int kStagePlane = 64 * kSlot;  // one limb plane of a half tile
constexpr size_t lds_bytes(int L) { return (size_t)L * kStagePlane * sizeof(uint32_t); }
}  // namespace rr

// bit masks of the bit-lanes p with bit j of p set (constexpr: callable from device code as it is)
constexpr uint32_t lane_mask(int j) {
	return j == 0 ? 0xAAAAAAAAu : j == 1 ? 0xCCCCCCCCu : j == 2 ? 0xF0F0F0F0u : j == 3 ? 0xFF00FF00u : 0xFFFF0000u;
}

// One pass = k consecutive stages lo..lo+k-1 over every tile. Passed by value as a kernel
// argument (~2.6 KB), so every table read is a scalar load from the kernarg segment. No kernel reads
// ob, two and twc any more (the tile's start comes from TileStart and the plan's chunk tables, below);
// they stay for the planner, plan_tile_starts and the host-only exports.
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

// The start of a tile (every pass kernel): what a work-group needs of its tile index before it can
// load the tile and run the stages, in a form that costs no serial table walk.
//   * The outer bits ob[] of a pass are at most two contiguous runs of index bits, so the packed
//     outer bits go to their index positions with two masks and shifts:
//       outer_off = (outer & mask[0]) << shift[0] | (outer & mask[1]) << shift[1]
//     (the bottom pass has one run: mask[1] = 0, and its kernels shift only).
//   * The work-group-uniform twiddle part of stage j is linear in x = outer | coset << n_outer. x is
//     cut into chunks of kChunkBits bits, and UT[c][v][j] holds the XOR of the two[j][.] / twc[j][.]
//     contributions of the set bits of chunk c's value v: the uniform part is the XOR over the
//     chunks of one row of kMaxStages words each. Chunks above n_chunks have the value 0, whose row is
//     zero in every chunk; a pass's tables always hold kMaxChunks chunks, so a kernel reads
//     kMaxChunks rows without a branch.
constexpr int kChunkBits = 6;
constexpr int kChunkRows = 1 << kChunkBits;
constexpr int kMaxChunks = 4;  // a plan has log_h + log_rate <= 32: at most 20 outer and coset bits
constexpr size_t kPassUtWords = (size_t)kMaxChunks * kChunkRows * kMaxStages;  // 12 KiB per pass
struct TileStart {
	uint32_t mask[2];
	int shift[2];
	int n_runs;                     // 0, 1 or 2: the pairs in use (a pair not in use has mask 0)
	int n_outer, n_bits, n_chunks;  // n_bits = n_outer + log_rate, n_chunks = ceil(n_bits / kChunkBits)
	uint32_t ut_word;               // first word of the pass's chunk tables in the plan's table buffer
};
// outer bits (packed) -> their index positions; what the kernels compute
constexpr size_t tile_outer_off(const TileStart& t, size_t outer) {
	return ((outer & t.mask[0]) << t.shift[0]) | ((outer & t.mask[1]) << t.shift[1]);
}
// The tile starts of a plan's passes and the chunk tables of all of them (`ut`, kPassUtWords words
// per pass, in pass order: the plan copies it to the device once). BN_ERR_UNSUPPORTED when a pass's
// outer bits are not two runs (checked bit by bit against ob[]), when the bottom pass has more than
// one run, or when outer and coset bits need more than kMaxChunks chunks.
int plan_tile_starts(int log_rate, const std::vector<BsPass>& passes, std::vector<TileStart>& starts, std::vector<uint32_t>& ut);

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

// ---- which kernel runs a launch. A family is one kernel template and the params struct it takes:
// antt_bs_pass, antt_bs3_pass (BsParams), antt_inv_bs_pass (InvBsParams), antt_rr_pass (RrParams)
enum class NttFamily { Bs, Bs3, InvBs, Rr };
// One instance: the family's template arguments (fmax 0: antt_bs3_pass<ROLE>; occ: antt_rr_pass only)
struct NttInstance {
	NttFamily family;
	int limbs, role, fmax, occ;
};
// Every pass kernel of the library: the .hip files instantiate from this list and nothing else, the
// plan sets the LDS attribute of each entry, and ntt_plan_launch returns an index into it. A plan
// holds FIRST at fmax 8 / 16 / 32, MID and LAST at 16 / 32, SINGLE at 16 (DESIGN.md section 5.1;
// tests/cpp/test_host_asan.cpp sweeps every plan). The LDS-tile kernels run fmax 16 on their GF(2^32)
// form; the inverse's roles are in its own order (its FIRST is the bottom pass).
constexpr NttInstance kNttInstances[] = {
    {NttFamily::Bs, 1, ROLE_FIRST, 8, 0},     {NttFamily::Bs, 4, ROLE_FIRST, 8, 0},
    {NttFamily::Bs, 1, ROLE_FIRST, 32, 0},    {NttFamily::Bs, 4, ROLE_FIRST, 32, 0},
    {NttFamily::Bs, 1, ROLE_MID, 32, 0},      {NttFamily::Bs, 4, ROLE_MID, 32, 0},
    {NttFamily::Bs, 1, ROLE_LAST, 32, 0},     {NttFamily::Bs, 4, ROLE_LAST, 32, 0},
    {NttFamily::Bs, 1, ROLE_SINGLE, 32, 0},   {NttFamily::Bs, 4, ROLE_SINGLE, 32, 0},
    {NttFamily::Bs3, 4, ROLE_FIRST, 0, 0},    {NttFamily::Bs3, 4, ROLE_MID, 0, 0},
    {NttFamily::InvBs, 1, ROLE_LAST, 8, 0},   {NttFamily::InvBs, 4, ROLE_LAST, 8, 0},
    {NttFamily::InvBs, 1, ROLE_LAST, 32, 0},  {NttFamily::InvBs, 4, ROLE_LAST, 32, 0},
    {NttFamily::InvBs, 1, ROLE_MID, 32, 0},   {NttFamily::InvBs, 4, ROLE_MID, 32, 0},
    {NttFamily::InvBs, 1, ROLE_FIRST, 32, 0}, {NttFamily::InvBs, 4, ROLE_FIRST, 32, 0},
    {NttFamily::InvBs, 1, ROLE_SINGLE, 32, 0}, {NttFamily::InvBs, 4, ROLE_SINGLE, 32, 0},
    {NttFamily::Rr, 1, ROLE_FIRST, 8, 1},     {NttFamily::Rr, 4, ROLE_FIRST, 8, 1},
    {NttFamily::Rr, 1, ROLE_FIRST, 16, 1},    {NttFamily::Rr, 4, ROLE_FIRST, 16, 1},
    {NttFamily::Rr, 1, ROLE_FIRST, 32, 1},    {NttFamily::Rr, 4, ROLE_FIRST, 32, 1},
    {NttFamily::Rr, 1, ROLE_MID, 16, 1},      {NttFamily::Rr, 4, ROLE_MID, 16, 1},
    {NttFamily::Rr, 1, ROLE_MID, 32, 1},      {NttFamily::Rr, 4, ROLE_MID, 32, 1},
    {NttFamily::Rr, 1, ROLE_LAST, 16, 3},     {NttFamily::Rr, 4, ROLE_LAST, 16, 3},
    {NttFamily::Rr, 1, ROLE_LAST, 32, 3},     {NttFamily::Rr, 4, ROLE_LAST, 32, 3},
    {NttFamily::Rr, 1, ROLE_SINGLE, 16, 3},   {NttFamily::Rr, 4, ROLE_SINGLE, 16, 3},
    // the bottom pass without the three-waves bound (no spills), for small launches
    {NttFamily::Rr, 4, ROLE_LAST, 16, 1},     {NttFamily::Rr, 4, ROLE_LAST, 32, 1},
};
constexpr int kNttInstanceCount = (int)(sizeof(kNttInstances) / sizeof(kNttInstances[0]));
// workgroup size and dynamic LDS bytes of an instance: its family's
constexpr unsigned instance_threads(const NttInstance& k) { return k.family == NttFamily::Bs3 ? kSplitNT : 64u * (unsigned)k.limbs; }
constexpr size_t instance_lds_bytes(const NttInstance& k) {
	return k.family == NttFamily::Rr ? rr::lds_bytes(k.limbs) : k.family == NttFamily::Bs3 ? kSplitLdsBytes : tile_lds_bytes(k.limbs);
}

// Kernel variants: 0 compact tiles (log_h < 12), 1 bitsliced LDS tiles (antt_bs_pass), 4 bitsliced
// register tiles (antt_rr_pass), 5 = 4 for the passes whose twiddles all lie in GF(2^8) (their kernel
// fits four waves per SIMD) and 1 for the others (the default for log_h >= 12).
constexpr bool valid_variant(int v) { return v == 0 || v == 1 || v == 4 || v == 5; }

// The environment switches of the development build (make BN_DEV=1), all of them; the product build
// reads none and has the defaults. They measure or select among kernels the product itself launches:
//   BN_DEBUG_FLAGS=bits  skip work for timing (wrong results): 1 no tile loads, 2 no tile stores,
//                        4 no multiplies (antt_bs_pass; antt_rr_pass takes bits 1 and 2, antt_bs3_pass bit 2)
//   BN_TRACE=1           per-wave phase times in cycles on stderr (antt_bs_pass, antt_bs3_pass; antt_rr_pass: its load phase)
//   BN_SPLIT=0/1         upper GF(2^16/32) passes never / always on the lane-split kernel
//   BN_RR_LAST=0         small bottom passes stay on LDS tiles
//   BN_ANTT_VARIANT=v    kernel variant of new plans with log_h >= 12 (1, 4 or 5)
struct BsDevKnobs {
	int dbg = 0, split = -1, rr_last = -1, variant = 5;
	bool trace = false;
};
BsDevKnobs bs_dev_knobs();

// One launch of a pass: workgroup b transforms tile b.
struct NttLaunch {
	int instance;  // index into kNttInstances; -1: the variant has no bitsliced passes
	size_t grid, lds;  // tiles, dynamic LDS bytes
	unsigned threads;
};
// What runs the pass of (the forward's) role `role` and largest stage field `fmax` over `ntiles` tiles
// on a device of `num_cus` compute units. The only place that decides it.
NttLaunch ntt_plan_launch(int limbs, int variant, bool inverse, int role, int fmax, size_t ntiles, int num_cus,
                          const BsDevKnobs& kn);

}  // namespace bn
