// Planning of the bit-reversal permutation of a GF(2^128) column (host only, bitrev_plan.cpp): the
// tile shape, the tile count, the launch shape, and the address functions of a tile. No HIP header:
// this is integer code, and the device side (bitrev.hip) includes this file for the constants and the
// address functions, so the kernel and the host-side sweep (tests/cpp/test_bitrev_plan.cpp) use the
// same ones.
//
// The n index bits are split as hi (q bits) | mid (m = n - 2q bits) | lo (q bits), and
//   rev_n(hi | mid | lo) = rev_q(lo) | rev_m(mid) | rev_q(hi).
// A tile is one value of mid in one transform of the batch: 2^(2q) elements. It is read as 2^q runs
// (one per hi) of 2^q consecutive elements and written as 2^q runs (one per rev_q(lo)) of 2^q
// consecutive elements, so with q >= 3 every global access is whole 128-byte lines. Position e of a
// tile's read order is (hi = e >> q, lo = e & (2^q - 1)); position e of its write order is
// (run = e >> q, pos = e & (2^q - 1)), which holds the element read at hi = rev_q(pos),
// lo = rev_q(run). q = min(tile_log or 6, n / 2): below n = 2q, mid has 0 bits or 1.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BN_BITREV_HD __host__ __device__
#else
#define BN_BITREV_HD
#endif

namespace bn {

constexpr int kBitrevMaxLog = 30;
constexpr int kBitrevTileLog = 6;     // q of a full tile: runs of 1 KiB, a tile of 64 KiB
constexpr int kBitrevThreadsLog = 9;  // 8 waves
constexpr int kBitrevThreads = 1 << kBitrevThreadsLog;
// elements of a full tile per thread: all of them are in flight before the first LDS write
constexpr int kBitrevPerThread = 1 << (2 * kBitrevTileLog - kBitrevThreadsLog);
constexpr size_t kBitrevLdsPerCu = 160 * 1024;
constexpr int kBitrevMaxWgsPerCu = 2048 / kBitrevThreads;  // the CU's 32 waves
constexpr uint64_t kBitrevMaxElems = (uint64_t)1 << 32;    // batch * 2^n

struct BitrevPlan {
	int n;             // index bits
	int q;             // bits of hi and of lo
	int m;             // bits of mid: n - 2q
	uint64_t n_tiles;  // batch << m
};

// False, with *plan untouched, unless 0 <= log_n <= kBitrevMaxLog, 0 <= tile_log <= kBitrevTileLog,
// batch >= 1 and batch << log_n <= kBitrevMaxElems.
bool bitrev_plan(int log_n, uint64_t batch, int tile_log, BitrevPlan* plan);

// the low `bits` bits of x reversed (bits <= 32; x < 2^bits)
BN_BITREV_HD inline uint32_t bitrev_rev(uint32_t x, int bits) {
#if defined(__HIP_DEVICE_COMPILE__)
	// what __brev is defined as (this header includes no HIP header): one v_bfrev_b32
	return bits ? __builtin_bitreverse32(x) >> (32 - bits) : 0u;
#else
	x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
	x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
	x = ((x >> 4) & 0x0f0f0f0fu) | ((x & 0x0f0f0f0fu) << 4);
	x = ((x >> 8) & 0x00ff00ffu) | ((x & 0x00ff00ffu) << 8);
	x = (x >> 16) | (x << 16);
	return bits ? x >> (32 - bits) : 0u;
#endif
}

BN_BITREV_HD inline uint32_t bitrev_tile_elems(const BitrevPlan& p) { return 1u << (2 * p.q); }

// element index (in the whole buffer of batch << n elements) of position e of tile t's read order
BN_BITREV_HD inline uint64_t bitrev_in_index(const BitrevPlan& p, uint64_t tile, uint32_t e) {
	const uint64_t b = tile >> p.m, mid = tile & (((uint64_t)1 << p.m) - 1);
	const uint64_t hi = e >> p.q, lo = e & ((1u << p.q) - 1);
	return (b << p.n) | (hi << (p.n - p.q)) | (mid << p.q) | lo;
}

// element index of position e of tile t's write order
BN_BITREV_HD inline uint64_t bitrev_out_index(const BitrevPlan& p, uint64_t tile, uint32_t e) {
	const uint64_t b = tile >> p.m;
	const uint32_t mid = (uint32_t)(tile & (((uint64_t)1 << p.m) - 1));
	const uint64_t run = e >> p.q, pos = e & ((1u << p.q) - 1);
	return (b << p.n) | (run << (p.n - p.q)) | ((uint64_t)bitrev_rev(mid, p.m) << p.q) | pos;
}

// The LDS slot (in elements) of the element read at (hi, lo). Rows are written as loaded (a wave:
// consecutive lo at one hi) and read transposed and reversed (a wave: one lo, hi = rev_q(pos) for
// consecutive pos). A row is 2^q * 16 B, 0 mod 64 dwords from q = 4 on, so unswizzled the 16 lanes
// of a ds_read_b128 group, which differ in the four highest bits of hi, would share one bank quad.
// XOR-ing those four bits into the column puts them on 16 different quads; a row write permutes
// within aligned groups of 16 slots and stays conflict-free. No padding: the tile is 2^(2q) slots.
BN_BITREV_HD inline uint32_t bitrev_lds_slot(int q, uint32_t hi, uint32_t lo) {
	const uint32_t sw = q >= 4 ? (hi >> (q - 4)) & 15u : hi;
	return (hi << q) | (lo ^ sw);
}

// position e of the write order reads this LDS slot
BN_BITREV_HD inline uint32_t bitrev_lds_read_slot(int q, uint32_t e) {
	return bitrev_lds_slot(q, bitrev_rev(e & ((1u << q) - 1), q), bitrev_rev(e >> q, q));
}

BN_BITREV_HD inline size_t bitrev_lds_bytes(int q) { return (size_t)16 << (2 * q); }

// work-groups: one per tile up to what the device holds at once (as many a CU as the LDS and the
// 32 waves allow: two at q = 6, four below); beyond that the work-groups stride over the tiles
inline uint64_t bitrev_grid(const BitrevPlan& p, int num_cus) {
	uint64_t per_cu = kBitrevLdsPerCu / bitrev_lds_bytes(p.q);
	if (per_cu > (uint64_t)kBitrevMaxWgsPerCu) per_cu = kBitrevMaxWgsPerCu;
	const uint64_t cap = (uint64_t)(num_cus > 0 ? num_cus : 256) * per_cu;
	return p.n_tiles < cap ? p.n_tiles : cap;
}

}  // namespace bn
