// Host-only sweep of the bit-reversal planner (binius-ntt_amd/csrc/bitrev_plan.cpp) and of the address
// functions the kernel uses (bitrev_plan.hpp), compiled with AddressSanitizer and UBSan by
// tests/test_bitrev_plan_host.py. No library, no GPU. For every (log_n, tile_log, batch):
//   - q = min(tile_log or 6, n / 2), mid has n - 2q bits, batch << (n - 2q) tiles;
//   - the tiles' read positions partition the index space, and so do their write positions
//     (enumerated up to 2^16 elements a transform; sampled tiles at 2^24 and 2^30);
//   - write position e holds the element read at (hi = rev(pos), lo = rev(run)), and its output
//     index is rev_n of that element's input index, in the same transform of the batch;
//   - every read run and every write run is 2^q consecutive elements aligned to min(2^q * 16, 128) B;
//   - the LDS slots of a tile are a bijection onto [0, 2^(2q)), the read slot of a write position is
//     the slot its element was written to, the bytes fit the per-CU budget the grid assumed, and from
//     q = 4 on neither the row writes (8 contiguous lanes, banks mod 32 dwords) nor the transposed
//     reads (the ds_read_b128 lane groups, banks mod 64 dwords) share a bank;
//   - the 64-bit indices do not wrap where a 32-bit shift would (2^32 elements).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "bitrev_plan.hpp"

using namespace bn;

static int failures = 0;
#define CHECK(cond, ...)                  \
	do {                                  \
		if (!(cond)) {                    \
			if (failures < 50) {          \
				std::printf("FAIL ");     \
				std::printf(__VA_ARGS__); \
				std::printf("\n");        \
			}                             \
			failures++;                   \
		}                                 \
	} while (0)

// written out bit by bit: what bitrev_rev must equal
static uint64_t rev_slow(uint64_t x, int bits) {
	uint64_t r = 0;
	for (int i = 0; i < bits; i++) r |= ((x >> i) & 1) << (bits - 1 - i);
	return r;
}

// the ds_read_b128 lane groups of a wave's lower half (the upper half is the same + 32)
static const int kReadGroup[2][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                      {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31}};

static void check_tile(const BitrevPlan& pl, uint64_t batch, uint64_t t, std::vector<uint8_t>* in_hit, std::vector<uint8_t>* out_hit) {
	const int n = pl.n, q = pl.q;
	const uint32_t E = bitrev_tile_elems(pl), R = 1u << q;
	const uint64_t N = (uint64_t)1 << n, total = batch << n;
	const uint64_t align_elems = R * 16 < 128 ? R : 8;  // min(2^q * 16, 128) bytes in elements
	for (uint32_t e = 0; e < E; e++) {
		const uint64_t xi = bitrev_in_index(pl, t, e), xo = bitrev_out_index(pl, t, e);
		CHECK(xi < total && xo < total, "n=%d q=%d tile %llu pos %u: index out of range", n, q, (unsigned long long)t, e);
		if (xi >= total || xo >= total) return;
		if (in_hit) (*in_hit)[xi]++;
		if (out_hit) (*out_hit)[xo]++;
		// runs
		if ((e & (R - 1)) == 0) {
			CHECK(xi % align_elems == 0 && xo % align_elems == 0, "n=%d q=%d tile %llu run %u: misaligned", n, q, (unsigned long long)t, e >> q);
		} else {
			CHECK(xi == bitrev_in_index(pl, t, e - 1) + 1 && xo == bitrev_out_index(pl, t, e - 1) + 1, "n=%d q=%d tile %llu pos %u: run broken",
			      n, q, (unsigned long long)t, e);
		}
		// the element a write position holds
		const uint32_t pos = e & (R - 1), run = e >> q;
		const uint32_t e_in = ((uint32_t)rev_slow(pos, q) << q) | (uint32_t)rev_slow(run, q);
		const uint64_t src = bitrev_in_index(pl, t, e_in);
		CHECK((src >> n) == (xo >> n) && (xo & (N - 1)) == rev_slow(src & (N - 1), n), "n=%d q=%d tile %llu pos %u: output is not rev_n of input", n,
		      q, (unsigned long long)t, e);
		CHECK(bitrev_lds_read_slot(q, e) == bitrev_lds_slot(q, e_in >> q, e_in & (R - 1)), "n=%d q=%d pos %u: read slot", n, q, e);
	}
}

static void check_lds(int q) {
	const uint32_t E = 1u << (2 * q), R = 1u << q;
	std::vector<uint8_t> hit(E, 0);
	for (uint32_t e = 0; e < E; e++) {
		const uint32_t s = bitrev_lds_slot(q, e >> q, e & (R - 1));
		CHECK(s < E, "q=%d pos %u: slot %u outside the tile", q, e, s);
		if (s < E) hit[s]++;
		CHECK(bitrev_lds_read_slot(q, e) < E, "q=%d pos %u: read slot outside the tile", q, e);
	}
	for (uint32_t s = 0; s < E; s++) CHECK(hit[s] == 1, "q=%d: slot %u written %d times", q, s, hit[s]);
	CHECK(bitrev_lds_bytes(q) == (size_t)E * 16 && 2 * bitrev_lds_bytes(q) <= kBitrevLdsPerCu, "q=%d: LDS bytes", q);
	if (q < 4) return;
	// a slot is 4 dwords: banks mod 32 dwords are slots mod 8, banks mod 64 dwords slots mod 16
	for (uint32_t e0 = 0; e0 < E; e0 += 8) {
		unsigned seen = 0;
		for (uint32_t l = 0; l < 8; l++) seen |= 1u << (bitrev_lds_slot(q, (e0 + l) >> q, (e0 + l) & (R - 1)) & 7);
		CHECK(seen == 0xff, "q=%d pos %u: row write shares a bank", q, e0);
	}
	for (uint32_t w0 = 0; w0 < E; w0 += 64)
		for (int half = 0; half < 2; half++)
			for (int g = 0; g < 2; g++) {
				unsigned seen = 0;
				for (int l = 0; l < 16; l++) seen |= 1u << (bitrev_lds_read_slot(q, w0 + 32 * half + kReadGroup[g][l]) & 15);
				CHECK(seen == 0xffff, "q=%d wave at %u: transposed read shares a bank", q, w0);
			}
}

static void sweep(int n, int tile_log, uint64_t batch) {
	BitrevPlan pl;
	CHECK(bitrev_plan(n, batch, tile_log, &pl), "bitrev_plan(%d, %llu, %d) rejected", n, (unsigned long long)batch, tile_log);
	const int cap = tile_log ? tile_log : kBitrevTileLog;
	CHECK(pl.n == n && pl.q == (n / 2 < cap ? n / 2 : cap) && pl.m == n - 2 * pl.q && pl.m >= 0, "n=%d tl=%d: q=%d m=%d", n, tile_log, pl.q, pl.m);
	CHECK(n >= 2 * cap || pl.m <= 1, "n=%d tl=%d: mid has %d bits below a full tile", n, tile_log, pl.m);
	CHECK(pl.n_tiles == batch << pl.m && pl.n_tiles * bitrev_tile_elems(pl) == batch << n, "n=%d tl=%d: %llu tiles", n, tile_log,
	      (unsigned long long)pl.n_tiles);
	CHECK(bitrev_tile_elems(pl) <= (uint32_t)kBitrevPerThread * kBitrevThreads, "n=%d tl=%d: a tile above a thread's share", n, tile_log);
	for (int cus : {0, 1, 256, 304}) {
		const uint64_t g = bitrev_grid(pl, cus), per_cu = g / (uint64_t)(cus > 0 ? cus : 256) + (g % (uint64_t)(cus > 0 ? cus : 256) != 0);
		CHECK(g >= 1 && g <= pl.n_tiles && g <= 0x7fffffffu, "n=%d tl=%d cus=%d: grid %llu", n, tile_log, cus, (unsigned long long)g);
		CHECK(per_cu <= (uint64_t)kBitrevMaxWgsPerCu && per_cu * bitrev_lds_bytes(pl.q) <= kBitrevLdsPerCu, "n=%d tl=%d cus=%d: LDS budget", n,
		      tile_log, cus);
	}
	if (n <= 16) {
		std::vector<uint8_t> in_hit(batch << n, 0), out_hit(batch << n, 0);
		for (uint64_t t = 0; t < pl.n_tiles; t++) check_tile(pl, batch, t, &in_hit, &out_hit);
		for (size_t i = 0; i < in_hit.size(); i++)
			CHECK(in_hit[i] == 1 && out_hit[i] == 1, "n=%d tl=%d: element %zu read %d times, written %d times", n, tile_log, i, in_hit[i], out_hit[i]);
	} else {
		// sampled: the first and the last tiles, and a stride through the middle
		std::vector<uint64_t> sample;
		for (uint64_t t = 0; t < 8 && t < pl.n_tiles; t++) sample.push_back(t);
		for (uint64_t t = 8; t + 8 < pl.n_tiles; t += pl.n_tiles / 61 + 1) sample.push_back(t);
		for (uint64_t t = pl.n_tiles > 8 ? pl.n_tiles - 8 : 0; t < pl.n_tiles; t++) sample.push_back(t);
		for (uint64_t t : sample) check_tile(pl, batch, t, nullptr, nullptr);
		// distinct tiles have distinct mid or batch bits: disjoint by construction of the index, checked on the end points
		CHECK(bitrev_in_index(pl, pl.n_tiles - 1, bitrev_tile_elems(pl) - 1) == (batch << n) - 1, "n=%d tl=%d: the last read is not the last element", n,
		      tile_log);
		CHECK(bitrev_out_index(pl, pl.n_tiles - 1, bitrev_tile_elems(pl) - 1) == (batch << n) - 1, "n=%d tl=%d: the last write is not the last element",
		      n, tile_log);
	}
}

int main() {
	for (int bits = 0; bits <= 32; bits++)
		for (uint64_t x : {0ull, 1ull, 2ull, 0x5ull, 0x12345678ull, 0xffffffffull}) {
			const uint64_t m = bits == 32 ? 0xffffffffull : ((1ull << bits) - 1);
			CHECK(bitrev_rev((uint32_t)(x & m), bits) == rev_slow(x & m, bits), "rev(%llx, %d)", (unsigned long long)(x & m), bits);
		}
	for (int q = 0; q <= kBitrevTileLog; q++) check_lds(q);
	for (int tl = 0; tl <= kBitrevTileLog; tl++) {
		for (int n = 0; n <= 16; n++)
			for (uint64_t batch : {1ull, 3ull}) sweep(n, tl, batch);
		sweep(24, tl, 1);
		sweep(24, tl, 3);
		sweep(30, tl, 1);
		sweep(30, tl, 4);  // 2^32 elements: byte offsets need 36 bits
	}
	BitrevPlan pl;
	CHECK(!bitrev_plan(-1, 1, 0, &pl) && !bitrev_plan(kBitrevMaxLog + 1, 1, 0, &pl), "log_n out of range accepted");
	CHECK(!bitrev_plan(8, 1, -1, &pl) && !bitrev_plan(8, 1, kBitrevTileLog + 1, &pl), "tile_log out of range accepted");
	CHECK(!bitrev_plan(8, 0, 0, &pl), "batch 0 accepted");
	CHECK(!bitrev_plan(30, 5, 0, &pl) && !bitrev_plan(0, ((uint64_t)1 << 32) + 1, 0, &pl) && bitrev_plan(0, (uint64_t)1 << 32, 0, &pl),
	      "the 2^32-element bound");
	CHECK(!bitrev_plan(8, ~(uint64_t)0, 0, &pl), "a batch that wraps accepted");
	CHECK(!bitrev_plan(8, 1, 0, nullptr), "NULL plan accepted");
	CHECK(bitrev_plan(24, 1, 0, &pl) && pl.q == 6 && pl.m == 12 && pl.n_tiles == 4096 && bitrev_grid(pl, 256) == 512, "2^24: 4096 tiles, two work-groups a CU");
	CHECK(bitrev_plan(13, 1, 5, &pl) && pl.q == 5 && pl.m == 3 && bitrev_grid(pl, 256) == 8, "2^13 at 2^5: 8 tiles");
	std::printf("%s (%d failures)\n", failures ? "FAILED" : "PASSED", failures);
	return failures ? 1 : 0;
}
