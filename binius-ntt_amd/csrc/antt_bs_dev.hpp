// Device helpers shared by the bitsliced kernels of the additive NTT: the forward LDS-tile passes
// (antt_bs.hip), the inverse passes (antt_inv.hip) and the register-tile passes (antt_rr.hip). Every
// piece of tile scaffolding has its one definition here: the tile's address bits, its twiddle tables,
// the LDS image and the two HBM layouts. Helpers that read only the field BsPass and RtPass share
// (bb) are templates on the pass table; the start of a tile (its address bits and the uniform parts of
// its twiddles) reads the pass's TileStart and the plan's chunk tables, not the pass table.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "antt_bs.hpp"
#include "bitsliced.hpp"
#include "bitsliced_ntt_gen.hpp"
#include "stream_io.hpp"  // ld_stream / st_stream: every byte is touched once per pass

namespace bn {

// out = w*x for 32 bitsliced GF(2^32) limbs (alias-safe: out may be x). W holds bit i of each
// lane's twiddle in word i; `field` (uniform per stage) selects the sub-field circuit, FMAX (the
// largest field of the pass) removes the circuits a pass never uses.
template <int FMAX>
__device__ __forceinline__ void mul_tw(int field, const uint32_t* x, const uint32_t* W, uint32_t* out) {
	if (FMAX <= 8 || field <= 8) {
#pragma unroll
		for (int g = 0; g < 4; g++) bsm3_mul(x + 8 * g, W, out + 8 * g);
	} else if (FMAX <= 16 || field <= 16) {
#pragma unroll
		for (int g = 0; g < 2; g++) bsm4_mul(x + 16 * g, W, out + 16 * g);
	} else {
		ntt_mul32(x, W, out);
	}
}

// (the LDS image of a tile, kPlane, and the kernels' LDS sizes: antt_passes.hpp)
constexpr int kLoads = kTileBlocks * 8 / 64;  // 16-byte global loads per lane per tile

// Words of a block stage's U that a lane requests from LDS next to V, ahead of the multiply circuit, so
// that their latency runs under it; the other words are read after the circuit. All 32 with the
// small GF(2^8) circuits and in the bottom pass (209-210 VGPRs). The upper GF(2^32) kernels have room
// for 16 (248-252 VGPRs): with 24 or 32 they reach 256 and spill.
constexpr int early_u_words(int role, int fmax) { return fmax <= 8 || role == ROLE_LAST ? 32 : 16; }

// Stage-to-stage ordering inside one wave: a wave's LDS operations execute in order, so only the
// compiler must not move accesses across this point (the wait also bounds the LDS queue).
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// ---- tile addressing. Workgroup b owns tile b = (outer bits, coset, batch); the tile's 128 blocks
// are the settings of the 7 index bits bb[], the outer bits ob[] are fixed per workgroup.
struct TileAddr {
	size_t outer;      // the n_outer fixed bits, packed
	int coset;         // < 2^log_rate
	size_t batch;
	size_t outer_off;  // the outer bits at their index positions (in blocks)
};
// (the inverse reads and writes one coset block: log_rate = 0, its coset is a launch parameter).
// Scalar shifts and ORs on the pass's TileStart (tile_outer_off), no table walk: nothing but the
// kernel's arguments stands ahead of the tile's first load. ONE_RUN: the bottom pass's outer bits are
// one run of index bits (plan_tile_starts checks it), a single shift. RUN_LOOP: see below
template <bool ONE_RUN = false, bool RUN_LOOP = false>
__device__ __forceinline__ TileAddr tile_addr(const TileStart& t, int log_rate) {
	const size_t tile = blockIdx.x;
	TileAddr a;
	a.outer = tile & (((size_t)1 << t.n_outer) - 1);
	const size_t rest = tile >> t.n_outer;
	a.coset = (int)(rest & ((1u << log_rate) - 1));
	a.batch = rest >> log_rate;
	if (ONE_RUN) {
		a.outer_off = a.outer << t.shift[0];
	} else if (!RUN_LOOP) {
		a.outer_off = tile_outer_off(t, a.outer);
	} else {
		// antt_rr_pass: tile_outer_off as a loop over the runs, both pairs in registers before it. With
		// the straight code, and nothing else changed, its upper instances lose a wave of occupancy
		// (<4, MID, 16>: 235 VGPRs against 168): the scheduler's occupancy target follows the block
		// structure ahead of the tile's loads
		uint32_t mask = t.mask[0], mask1 = t.mask[1];
		int shift = t.shift[0], shift1 = t.shift[1];
		a.outer_off = 0;
#pragma unroll 1
		for (int r = 0; r < t.n_runs; r++) {
			a.outer_off |= (a.outer & mask) << shift;
			mask = mask1, shift = shift1;
		}
	}
	return a;
}
// tile block q -> its index bits
template <class Pass>
__device__ __forceinline__ size_t tile_off(const Pass& ps, int q) {
	size_t off = 0;
#pragma unroll
	for (int m = 0; m < kBlkBits; m++) off |= (size_t)((q >> m) & 1) << ps.bb[m];
	return off;
}
// HBM word offsets inside a transform of L-limb elements, blocks in element order:
// 16-byte piece u of the tile in compact (AoS) elements, 8*L pieces per 32-element block
template <int L, class Pass>
__device__ __forceinline__ size_t compact_off(const Pass& ps, size_t outer_off, int u) {
	return (outer_off | tile_off(ps, u / (8 * L))) * L + 4 * (u % (8 * L));
}
// 16-byte chunk j of limb l of tile block q in bitsliced blocks (a limb of a block: 128 contiguous bytes)
template <int L, class Pass>
__device__ __forceinline__ size_t bitsliced_off(const Pass& ps, size_t outer_off, int q, int l, int j) {
	return (outer_off | tile_off(ps, q)) * L + 32 * l + 4 * j;
}

// ---- twiddles: linear in the index bits, tabulated per stage j of the pass.
// Workgroup-uniform part (outer and coset bits) of every stage: the XOR of one row of the pass's
// chunk tables per chunk of x = outer | coset << n_outer (TileStart, antt_passes.hpp). The row
// addresses are wave-uniform and the tables never change after the plan is prepared, so the rows come
// through the constant address space as scalar loads, all kMaxChunks of them in flight at once
// behind one wait, and are XORed on the scalar unit (uniform_tw_rows: stage j's word in u[j]): no
// vector-memory instruction, so the only vmcnt a tile's start waits on is its own data's. `ut` is the
// plan's table buffer. uniform_tw_to_lanes hands stage j's word to lane j.
typedef const uint32_t __attribute__((address_space(4))) * ConstWords;
__device__ __forceinline__ void uniform_tw_rows(const TileStart& t, const uint32_t* ut, size_t outer, int coset, uint32_t* u) {
	const uint32_t x = (uint32_t)outer | ((uint32_t)coset << t.n_outer);
	const ConstWords tab = (ConstWords)(uintptr_t)(ut + t.ut_word);
#pragma unroll
	for (int j = 0; j < kMaxStages; j++) u[j] = 0;
#pragma unroll
	for (int c = 0; c < kMaxChunks; c++) {
		const ConstWords row = tab + ((uint32_t)(c * kChunkRows) + ((x >> (kChunkBits * c)) & (kChunkRows - 1))) * kMaxStages;
#pragma unroll
		for (int j = 0; j < kMaxStages; j++) u[j] ^= row[j];
	}
}
__device__ __forceinline__ uint32_t uniform_tw_to_lanes(const uint32_t* u) {
	uint32_t v = 0;
#pragma unroll
	for (int j = 0; j < kMaxStages; j++) asm("v_writelane_b32 %0, %1, %2" : "+v"(v) : "s"(u[j]), "n"(j));
	return v;
}
__device__ __forceinline__ uint32_t uniform_tw_lanes(const TileStart& t, const uint32_t* ut, size_t outer, int coset) {
	uint32_t u[kMaxStages];
	uniform_tw_rows(t, ut, outer, coset, u);
	return uniform_tw_to_lanes(u);
}
// part of tile block q
__device__ __forceinline__ uint32_t tile_tw(const BsPass& ps, int j, int q) {
	uint32_t w = 0;
#pragma unroll
	for (int m = 0; m < kBlkBits; m++) w ^= ps.twt[j][m] & (uint32_t)__builtin_amdgcn_sbfe(q, m, 1);
	return w;
}
// The stage on the top tile bit: the block pair's bits 0..5 are the lane's, and when none of them
// moves the twiddle (twt[j][0..5] = 0: the tile's other bits are lower stages) it is the
// workgroup-uniform part alone, so the circuit's twiddle side is scalar (ntt_mul32_w)
template <int FMAX>
__device__ __forceinline__ bool top_stage_uniform(const BsPass& ps, int j, int m) {
	uint32_t lane_part = 0;
#pragma unroll
	for (int mm = 0; mm < kBlkBits - 1; mm++) lane_part |= ps.twt[j][mm];
	return FMAX == 32 && m == kBlkBits - 1 && ps.field[j] == 32 && lane_part == 0u;
}
// twiddle words of a circuit: word i = bit i of the twiddle w in every bit-lane, XOR the bit-lane
// part `pat` of an in-word stage (nullptr: none)
template <int N = 32>
__device__ __forceinline__ void tw_words(uint32_t w, const uint32_t* pat, uint32_t* W) {
#pragma unroll
	for (int i = 0; i < N; i++) W[i] = (pat ? pat[i] : 0u) ^ (uint32_t)__builtin_amdgcn_sbfe(w, i, 1);
}

// ---- the LDS image. Word `word` of the L-limb compact element row of block q: limb word % L
template <int L>
__device__ __forceinline__ uint32_t* plane_word(uint32_t* lds, int q, int word) {
	return lds + (word % L) * kPlane + q * kLimbStride + word / L;
}
// compact 16-byte piece u of the tile (compact_off) scattered into / gathered from the limb planes
template <int L>
__device__ __forceinline__ void compact_to_planes(uint32_t* lds, int u, uint4 g) {
	const int q = u / (8 * L), j = u % (8 * L);
	const uint32_t w[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
	for (int t = 0; t < 4; t++) *plane_word<L>(lds, q, 4 * j + t) = w[t];
}
template <int L>
__device__ __forceinline__ uint4 planes_to_compact(uint32_t* lds, int u) {
	const int q = u / (8 * L), j = u % (8 * L);
	uint32_t w[4];
#pragma unroll
	for (int t = 0; t < 4; t++) w[t] = *plane_word<L>(lds, q, 4 * j + t);
	return make_uint4(w[0], w[1], w[2], w[3]);
}
// 32x32 bit transpose of a block held in LDS (compact words <-> bitsliced words of one limb)
__device__ __forceinline__ void transpose_block(uint32_t* x) {
	uint32_t r[32];
#pragma unroll
	for (int i = 0; i < 32; i += 4) *(uint4*)(r + i) = *(const uint4*)(x + i);
	transpose32(r);
#pragma unroll
	for (int i = 0; i < 32; i += 4) *(uint4*)(x + i) = *(const uint4*)(r + i);
}

// ---- bitsliced tile I/O of one wave: its limb plane l, piece u = lane + 64 r of the plane being
// chunk u & 7 of block u >> 3. skip_* are the timing switches of the development build (no loads /
// no stores, wrong results).
// The lane's piece r of the plane from HBM; the caller issues all kLoads of them before anything
// waits (the loop stays in the kernel: with the register array passed into a helper the inverse's
// top pass takes 255 VGPRs against 195).
// CONTIG: the bottom pass's tile (bb[m] = 5 + m) is one contiguous run of 2^12 elements at outer_off:
// a workgroup-uniform base and a 32-bit offset per lane
template <int L, bool CONTIG = false, class Pass>
__device__ __forceinline__ uint4 load_plane_bitsliced(const Pass& ps, const uint32_t* src, size_t outer_off, int l,
                                                      int lane, int r, bool skip_loads = false) {
	const int u = lane + r * 64;
	const int q = u >> 3, j = u & 7;
	const uint32_t* g = CONTIG ? src + outer_off * L + (uint32_t)(q * 32 * L + 32 * l + 4 * j) : src + bitsliced_off<L>(ps, outer_off, q, l, j);
	return skip_loads ? make_uint4(u, j, q, 64 * l + lane) : ld_stream(g);
}
__device__ __forceinline__ void plane_from_regs(uint32_t* plane, int lane, const uint4* gbuf) {
#pragma unroll
	for (int r = 0; r < kLoads; r++) {
		const int u = lane + r * 64;
		*(uint4*)(plane + (u >> 3) * kLimbStride + 4 * (u & 7)) = gbuf[r];
	}
}
template <int L, class Pass>
__device__ __forceinline__ void store_plane_bitsliced(const Pass& ps, uint32_t* dst, size_t outer_off, int l, int lane,
                                                      const uint32_t* plane, bool skip_stores = false) {
#pragma unroll 4
	for (int r = 0; r < kLoads; r++) {
		const int u = lane + r * 64;
		const int q = u >> 3, j = u & 7;
		const uint4 g = *(const uint4*)(plane + q * kLimbStride + 4 * j);
		if (!skip_stores) st_stream(dst + bitsliced_off<L>(ps, outer_off, q, l, j), g);
	}
}

}  // namespace bn
