// Host-only sweep of the Merkle commitment's pass planner (binius-ntt_amd/csrc/merkle_plan.cpp) and of
// the address functions the kernels use (merkle_plan.hpp), compiled with AddressSanitizer and UBSan by
// tests/test_merkle_plan_host.py. No library, no GPU. For every (log_leaves, log_leaf_elems, cap):
//   - the passes write rows 0 .. L once each and in order; one leaf pass, first; at most one tail, last;
//   - the groups of a pass read a partition of the row they read, and the nodes they write into each
//     row partition that row: no range leaves its row, every node is written once (enumerated up to
//     2^16 nodes a row, by the groups' end points above that);
//   - a group never has more items than its LDS planes hold, a pass's last row has at least one node
//     a group, and outside forced caps every fused row fills whole waves;
//   - the LDS fits, and the 64-bit offsets do not wrap (L = 30).
// And the host SHA-256 on the FIPS 180-4 vectors "" and "abc", the node rule's known answer, and
// mk_verify on a small tree built with the host functions.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "merkle_plan.hpp"

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

static void sweep(int L, int a, int max_rows) {
	MkPlan pl;
	CHECK(mk_plan(L, a, max_rows, &pl), "mk_plan(%d, %d, %d) rejected", L, a, max_rows);
	CHECK(pl.n_passes >= 1 && pl.n_passes <= kMkMaxPasses, "L=%d cap=%d: %d passes", L, max_rows, pl.n_passes);
	const int cap = max_rows ? max_rows : kMkRowsPerPass, tail_cap = max_rows ? max_rows : kMkTailRows;
	int next_row = 0;
	for (int p = 0; p < pl.n_passes; p++) {
		const MkPass& ps = pl.pass[p];
		CHECK(ps.first_row == next_row && ps.rows >= 1, "L=%d cap=%d pass %d: rows %d+%d after %d", L, max_rows, p, ps.first_row, ps.rows, next_row);
		next_row = ps.first_row + ps.rows;
		CHECK((ps.kind == kMkLeaf) == (p == 0), "L=%d cap=%d pass %d: the leaf pass is the first and only the first", L, max_rows, p);
		CHECK(ps.kind != kMkTail || p == pl.n_passes - 1, "L=%d cap=%d pass %d: the tail is not last", L, max_rows, p);
		CHECK(ps.rows <= (ps.kind == kMkTail ? tail_cap : cap), "L=%d cap=%d pass %d: %d rows", L, max_rows, p, ps.rows);

		const int group_log = ps.kind == kMkLeaf ? kMkLeafGroupLog : kMkRowGroupLog;
		const int row_in = ps.kind == kMkLeaf ? 0 : ps.first_row - 1;
		const int steps = ps.kind == kMkLeaf ? ps.rows - 1 : ps.rows;  // node rows: row_in + 1 .. row_in + steps
		const uint64_t groups = mk_groups(L, row_in, group_log);
		const uint32_t items = mk_group_items(L, row_in, group_log);
		CHECK(ps.kind != kMkTail || groups == 1, "L=%d cap=%d: the tail has %llu groups", L, max_rows, (unsigned long long)groups);
		CHECK(items <= (1u << group_log) && groups * items == mk_row_nodes(L, row_in), "L=%d cap=%d pass %d: groups x items != the row", L,
		      max_rows, p);
		CHECK(groups <= 0x7fffffffull, "L=%d cap=%d pass %d: grid", L, max_rows, p);
		CHECK(row_in + steps <= L, "L=%d cap=%d pass %d: writes past the root", L, max_rows, p);
		for (int k = 1; k <= steps; k++) {
			const uint32_t n = mk_group_nodes(L, row_in, group_log, k);
			const uint64_t row_nodes = mk_row_nodes(L, row_in + k);
			CHECK(n >= 1 && n <= (uint32_t)kMkThreads, "L=%d cap=%d pass %d step %d: %u nodes a group", L, max_rows, p, k, n);
			CHECK(n * groups == row_nodes, "L=%d cap=%d pass %d step %d: the groups do not make up the row", L, max_rows, p, k);
			if (max_rows == 0 && ps.kind != kMkTail) CHECK(n % 64 == 0, "L=%d pass %d step %d: %u nodes do not fill waves", L, p, k, n);
			// planes: step k reads n * 2 entries of one buffer and writes n of the other
			CHECK(2 * n <= (k % 2 ? 1u << group_log : 1u << (group_log - 1)), "L=%d cap=%d pass %d step %d: planes too short", L, max_rows, p, k);
			// end points of the groups: every group up to 2^12 and the last ones beyond
			for (uint64_t g = 0; g < groups; g = (g == 4095 && groups > 8192 ? groups - 4096 : g + 1)) {
				const uint64_t first = mk_group_first_node(L, row_in, group_log, k, g);
				CHECK(first == g * n && first + n <= row_nodes, "L=%d cap=%d pass %d step %d group %llu: leaves its row", L, max_rows, p, k,
				      (unsigned long long)g);
				const uint64_t at = mk_row_offset(L, row_in + k) + first;
				CHECK(at + n <= mk_tree_digests(L), "L=%d cap=%d pass %d step %d group %llu: past the tree", L, max_rows, p, k, (unsigned long long)g);
			}
			if (row_nodes <= (1u << 16)) {
				std::vector<uint8_t> hit(row_nodes, 0);
				for (uint64_t g = 0; g < groups; g++)
					for (uint32_t t = 0; t < n; t++) {
						const uint64_t i = mk_group_first_node(L, row_in, group_log, k, g) + t;
						CHECK(i < row_nodes, "L=%d cap=%d pass %d step %d: node outside its row", L, max_rows, p, k);
						if (i < row_nodes) hit[i]++;
					}
				for (size_t i = 0; i < hit.size(); i++) CHECK(hit[i] == 1, "L=%d cap=%d pass %d step %d: node %zu written %d times", L, max_rows, p, k, i, hit[i]);
			}
		}
	}
	CHECK(next_row == L + 1, "L=%d cap=%d: rows up to %d written", L, max_rows, next_row - 1);
	// rows in the buffer: consecutive, the root last
	uint64_t at = 0;
	for (int h = 0; h <= L; h++) {
		CHECK(mk_row_offset(L, h) == at, "L=%d: row %d at %llu, expected %llu", L, h, (unsigned long long)mk_row_offset(L, h), (unsigned long long)at);
		at += mk_row_nodes(L, h);
	}
	CHECK(at == mk_tree_digests(L) && mk_row_offset(L, L) == mk_tree_digests(L) - 1, "L=%d: the root is not the last digest", L);
	CHECK(mk_open_bytes(L, a) == ((uint64_t)16 << a) + 32u * L, "L=%d a=%d: record bytes", L, a);
	CHECK((size_t)mk_leaf_lds_words(a) * 4 <= kMkLdsPerGroup && (size_t)mk_row_lds_words() * 4 <= kMkLdsPerGroup, "a=%d: LDS", a);
	// the stage: 64 rows a wave, a row holds the chunk; the digest planes fit in the same LDS
	CHECK(mk_stage_row_words(a) >= 4u * mk_chunk_vecs(a) && (1 << a) % mk_chunk_vecs(a) == 0, "a=%d: stage rows", a);
	CHECK(mk_leaf_lds_words(a) >= (uint32_t)kMkThreads * mk_stage_row_words(a) && mk_leaf_lds_words(a) >= mk_digest_lds_words(kMkThreads),
	      "a=%d: leaf LDS", a);
}

static bool hex_is(const uint8_t d[32], const char* hex) {
	char buf[65];
	for (int i = 0; i < 32; i++) std::snprintf(buf + 2 * i, 3, "%02x", d[i]);
	return std::strcmp(buf, hex) == 0;
}

static void hashes() {
	uint8_t d[32];
	sha256_hash((const uint8_t*)"", 0, d);
	CHECK(hex_is(d, "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855"), "SHA-256 of the empty message");
	sha256_hash((const uint8_t*)"abc", 3, d);
	CHECK(hex_is(d, "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"), "SHA-256 of abc");
	// 56 bytes: the padding spills into a second block
	sha256_hash((const uint8_t*)"abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq", 56, d);
	CHECK(hex_is(d, "248d6a61d20638b8e5c026930c3e6039a33ce45964ff2167f6ecedd419db06c1"), "SHA-256 of the 56-byte vector");
	const uint8_t zero[32] = {0};
	mk_hash_node(zero, zero, d);
	CHECK(hex_is(d, "da5698be17b9b46962335799779fbeca8ce5d491c0d26243bafef9ea1837a9d8"), "node of two all-zero children");

	// a tree of 8 leaves of 4 elements built with the host functions; every record verifies, a tampered one does not
	const int L = 3, a = 2;
	std::vector<uint8_t> data((size_t)16 << (L + a));
	for (size_t i = 0; i < data.size(); i++) data[i] = (uint8_t)(i * 37 + (i >> 5));
	std::vector<uint8_t> tree(32 * mk_tree_digests(L));
	for (int j = 0; j < 1 << L; j++) mk_hash_leaf(&data[(size_t)j * (16 << a)], a, &tree[32 * j]);
	for (int h = 1; h <= L; h++)
		for (uint64_t k = 0; k < mk_row_nodes(L, h); k++)
			mk_hash_node(&tree[32 * (mk_row_offset(L, h - 1) + 2 * k)], &tree[32 * (mk_row_offset(L, h - 1) + 2 * k + 1)],
			             &tree[32 * (mk_row_offset(L, h) + k)]);
	const uint8_t* root = &tree[32 * (mk_tree_digests(L) - 1)];
	for (uint64_t j = 0; j < (1u << L); j++) {
		std::vector<uint8_t> rec(mk_open_bytes(L, a));
		std::memcpy(rec.data(), &data[j * (16 << a)], 16 << a);
		for (int h = 0; h < L; h++) std::memcpy(&rec[(16 << a) + 32 * h], &tree[32 * (mk_row_offset(L, h) + ((j >> h) ^ 1))], 32);
		CHECK(mk_verify(root, L, a, j, rec.data()), "record %llu rejected", (unsigned long long)j);
		CHECK(!mk_verify(root, L, a, j ^ 1, rec.data()) && !mk_verify(root, L, a, j + 8, rec.data()), "record %llu accepted at a wrong index", (unsigned long long)j);
		rec[(j * 11) % rec.size()] ^= 0x10;
		CHECK(!mk_verify(root, L, a, j, rec.data()), "tampered record %llu accepted", (unsigned long long)j);
	}
}

int main() {
	MkPlan pl;
	for (int a = 0; a <= kMkMaxLeafLog; a++)
		for (int L = 0; L + a <= kMkMaxLogElems; L++)
			for (int cap = 0; cap <= kMkRowsPerPass; cap++) sweep(L, a, cap);
	CHECK(!mk_plan(-1, 0, 0, &pl) && !mk_plan(31, 0, 0, &pl) && !mk_plan(23, 8, 0, &pl), "log_leaves out of range accepted");
	CHECK(!mk_plan(4, -1, 0, &pl) && !mk_plan(4, 9, 0, &pl), "log_leaf_elems out of range accepted");
	CHECK(!mk_plan(8, 2, -1, &pl) && !mk_plan(8, 2, kMkRowsPerPass + 1, &pl), "cap out of range accepted");
	CHECK(!mk_plan(8, 2, 0, nullptr), "NULL plan accepted");
	CHECK(mk_plan(0, 4, 0, &pl) && pl.n_passes == 1 && pl.pass[0].kind == kMkLeaf && pl.pass[0].rows == 1, "L = 0 is the leaf pass alone");
	CHECK(mk_plan(30, 0, 1, &pl) && pl.n_passes == 31 && pl.n_passes <= kMkMaxPasses, "L = 30 at cap 1 is the longest plan: 1 + 29 + 1 passes");
	// 32-byte digests: the root's byte offset at L = 30 needs 37 bits, which is why the offsets are 64-bit
	CHECK((32 * mk_row_offset(30, 30)) >> 32 == 15, "L=30: byte offset of the root");
	hashes();
	std::printf("%s (%d failures)\n", failures ? "FAILED" : "PASSED", failures);
	return failures ? 1 : 0;
}
