// Stand-alone host test of the tile-start tables of the additive NTT's pass kernels
// (plan_tile_starts, binius-ntt_amd/csrc/antt_passes.cpp): links antt_passes.cpp only, built with
// AddressSanitizer and UBSan by tests/test_tile_tables_host.py.
//
// Over all 95 plans (log_rate 0..4, log_h 12 .. 32 - log_rate) and every pass of each:
//   * the closed-form outer offset (tile_outer_off: two masks and shifts) equals the bit-by-bit
//     deposit of the packed outer bits into ob[];
//   * the XOR of one chunk-table row per chunk equals the bit-by-bit sum over two[j][.] / twc[j][.]
//     for every stage j, for every coset value;
//   * chunk count, table offsets and the buffer size stay inside their stated bounds.
// Tile indices (outer values) per pass: all of them up to 2^12, otherwise 0, all-ones, every one-hot
// and 4096 seeded random ones.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "antt_passes.hpp"
#include "binius_ntt_amd.h"

// the one symbol antt_passes.cpp needs from the rest of the library
namespace bn {
void set_error(const char* fmt, ...) {
	va_list ap;
	va_start(ap, fmt);
	vfprintf(stderr, fmt, ap);
	va_end(ap);
	fputc('\n', stderr);
}
}  // namespace bn

using namespace bn;

static int failures = 0;
#define CHECK(cond, ...)                 \
	do {                                 \
		if (!(cond)) {                   \
			if (failures++ < 20) {       \
				printf("FAIL: " __VA_ARGS__); \
				printf("\n");            \
			}                            \
		}                                \
	} while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {  // splitmix64
	uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}

// what the parent's kernels computed: tile_addr's loop and uniform_tw's two loops
static size_t deposit(const BsPass& p, size_t outer) {
	size_t off = 0;
	for (int m = 0; m < p.n_outer; m++) off |= ((outer >> m) & 1) << p.ob[m];
	return off;
}
static uint32_t uniform_tw_bits(const BsPass& p, int j, size_t outer, int coset) {
	uint32_t c = 0;
	for (int m = 0; m < p.n_outer; m++) c ^= p.two[j][m] & (0u - (uint32_t)((outer >> m) & 1));
	for (int b = 0; b < kMaxRateBits; b++) c ^= p.twc[j][b] & (0u - (uint32_t)((coset >> b) & 1));
	return c;
}
// what the new kernels compute: kMaxChunks rows, whatever n_chunks is
static void uniform_tw_rows(const TileStart& t, const std::vector<uint32_t>& ut, size_t outer, int coset, uint32_t* out) {
	const size_t x = outer | ((size_t)coset << t.n_outer);
	for (int j = 0; j < kMaxStages; j++) out[j] = 0;
	for (int c = 0; c < kMaxChunks; c++) {
		const size_t v = (x >> (kChunkBits * c)) & (kChunkRows - 1);
		const size_t row = (size_t)t.ut_word + ((size_t)c * kChunkRows + v) * kMaxStages;
		if (row + kMaxStages > ut.size()) {
			CHECK(false, "row %zu past the buffer (%zu words)", row, ut.size());
			return;
		}
		for (int j = 0; j < kMaxStages; j++) out[j] ^= ut[row + j];
	}
}

static void check_tile(int log_h, int r, size_t i, const BsPass& p, const TileStart& t, const std::vector<uint32_t>& ut, size_t outer) {
	CHECK(tile_outer_off(t, outer) == deposit(p, outer), "outer_off: log_h %d rate %d pass %zu outer %zx: %zx != %zx", log_h, r, i,
	      outer, tile_outer_off(t, outer), deposit(p, outer));
	const bool bottom = p.role == ROLE_LAST || p.role == ROLE_SINGLE;
	if (bottom) CHECK(outer << t.shift[0] == deposit(p, outer), "bottom pass: outer_off is not one shift (log_h %d rate %d)", log_h, r);
	for (int coset = 0; coset < (1 << r); coset++) {
		uint32_t got[kMaxStages];
		uniform_tw_rows(t, ut, outer, coset, got);
		for (int j = 0; j < kMaxStages; j++) {
			const uint32_t want = j < p.k ? uniform_tw_bits(p, j, outer, coset) : 0u;
			CHECK(got[j] == want, "uniform twiddle: log_h %d rate %d pass %zu stage %d outer %zx coset %d: %08x != %08x", log_h, r, i, j,
			      outer, coset, got[j], want);
		}
	}
}

int main() {
	static_assert(kMaxChunks <= 5, "stated bound: at most 5 chunks");
	static_assert(kPassUtWords * sizeof(uint32_t) < 16384, "stated bound: under 16 KiB of chunk tables per pass");
	static_assert(kMaxChunks * kChunkBits >= 32 - kMinLogH, "every plan's outer and coset bits fit the chunks");
	int plans = 0;
	size_t tiles = 0;
	for (int r = 0; r <= 4; r++)
		for (int log_h = kMinLogH; log_h <= 32 - r; log_h++) {
			plans++;
			std::vector<uint32_t> s, ut;
			std::vector<BsPass> passes;
			std::vector<RtPass> rt;
			std::vector<TileStart> starts;
			subspace_evals(log_h, r, s);
			if (!bs_supports(log_h, r) || plan_pass_tables(log_h, r, s, passes, rt) != BN_OK ||
			    plan_tile_starts(r, passes, starts, ut) != BN_OK) {
				CHECK(false, "log_h %d rate %d: no plan", log_h, r);
				continue;
			}
			CHECK(starts.size() == passes.size() && ut.size() == passes.size() * kPassUtWords, "log_h %d rate %d: sizes", log_h, r);
			CHECK(ut.size() * sizeof(uint32_t) <= 4 * 16384, "log_h %d rate %d: %zu table words", log_h, r, ut.size());
			for (size_t i = 0; i < passes.size(); i++) {
				const BsPass& p = passes[i];
				const TileStart& t = starts[i];
				CHECK(t.n_outer == p.n_outer && t.n_bits == p.n_outer + r, "log_h %d rate %d pass %zu: bit counts", log_h, r, i);
				CHECK(t.n_chunks == (t.n_bits + kChunkBits - 1) / kChunkBits && t.n_chunks <= kMaxChunks && t.n_chunks <= 5,
				      "log_h %d rate %d pass %zu: %d chunks", log_h, r, i, t.n_chunks);
				CHECK(t.ut_word == i * kPassUtWords, "log_h %d rate %d pass %zu: table offset", log_h, r, i);
				CHECK((t.mask[0] & t.mask[1]) == 0 && ((uint64_t)t.mask[0] | t.mask[1]) == ((uint64_t)1 << p.n_outer) - 1,
				      "log_h %d rate %d pass %zu: masks %x %x", log_h, r, i, t.mask[0], t.mask[1]);
				// the zero row of every chunk, used chunk or not
				for (int c = 0; c < kMaxChunks; c++)
					for (int j = 0; j < kMaxStages; j++)
						CHECK(ut[t.ut_word + (size_t)c * kChunkRows * kMaxStages + j] == 0, "log_h %d rate %d pass %zu: zero row", log_h, r, i);
				const size_t n_tiles = (size_t)1 << p.n_outer;
				if (p.n_outer <= 12) {
					for (size_t o = 0; o < n_tiles; o++) check_tile(log_h, r, i, p, t, ut, o);
					tiles += n_tiles;
				} else {
					check_tile(log_h, r, i, p, t, ut, 0);
					check_tile(log_h, r, i, p, t, ut, n_tiles - 1);
					for (int m = 0; m < p.n_outer; m++) check_tile(log_h, r, i, p, t, ut, (size_t)1 << m);
					for (int k = 0; k < 4096; k++) check_tile(log_h, r, i, p, t, ut, (size_t)(rng() & (n_tiles - 1)));
					tiles += 2 + (size_t)p.n_outer + 4096;
				}
			}
		}
	CHECK(plans == 95, "%d plans", plans);
	printf("%d plans, %zu tile indices\n", plans, tiles);
	printf("%s (%d failures)\n", failures ? "FAILED" : "PASSED", failures);
	return failures ? 1 : 0;
}
