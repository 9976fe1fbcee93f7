// Pass planner and host SHA-256 of the Merkle commitment (host only; see merkle_plan.hpp).
#include "merkle_plan.hpp"

#include <string.h>

namespace bn {

bool mk_plan(int log_leaves, int log_leaf_elems, int max_rows, MkPlan* plan) {
	if (plan == nullptr || log_leaf_elems < 0 || log_leaf_elems > kMkMaxLeafLog) return false;
	if (log_leaves < 0 || log_leaves + log_leaf_elems > kMkMaxLogElems) return false;
	if (max_rows < 0 || max_rows > kMkRowsPerPass) return false;
	const int cap = max_rows ? max_rows : kMkRowsPerPass;
	const int tail_cap = max_rows ? max_rows : kMkTailRows;
	MkPlan pl{};
	// the leaf pass goes on to the next rows only while its work-groups are full
	int fused = log_leaves >= kMkLeafGroupLog ? cap - 1 : 0;
	if (fused > log_leaves) fused = log_leaves;
	pl.pass[pl.n_passes++] = MkPass{kMkLeaf, 0, 1 + fused};
	int top = fused;  // the highest row written so far
	const int left = log_leaves - top;
	const int tail = left < tail_cap ? left : tail_cap;
	int mid = left - tail;  // rows of the row passes, the first pass taking the remainder
	while (mid > 0) {
		const int rows = mid % cap ? mid % cap : cap;
		pl.pass[pl.n_passes++] = MkPass{kMkRow, top + 1, rows};
		top += rows;
		mid -= rows;
	}
	if (tail > 0) pl.pass[pl.n_passes++] = MkPass{kMkTail, top + 1, tail};
	*plan = pl;
	return true;
}

static inline uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

void sha256_compress(uint32_t state[8], const uint8_t block[64]) {
	uint32_t w[64];
	for (int i = 0; i < 16; i++)
		w[i] = (uint32_t)block[4 * i] << 24 | (uint32_t)block[4 * i + 1] << 16 | (uint32_t)block[4 * i + 2] << 8 | block[4 * i + 3];
	for (int i = 16; i < 64; i++) {
		const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
		const uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
		w[i] = w[i - 16] + s0 + w[i - 7] + s1;
	}
	uint32_t a = state[0], b = state[1], c = state[2], d = state[3], e = state[4], f = state[5], g = state[6], h = state[7];
	for (int i = 0; i < 64; i++) {
		const uint32_t t1 = h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + kSha256K[i] + w[i];
		const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
		h = g, g = f, f = e, e = d + t1, d = c, c = b, b = a, a = t1 + t2;
	}
	state[0] += a, state[1] += b, state[2] += c, state[3] += d, state[4] += e, state[5] += f, state[6] += g, state[7] += h;
}

static void put_state(const uint32_t state[8], uint8_t out[32]) {
	for (int i = 0; i < 8; i++) {
		out[4 * i] = (uint8_t)(state[i] >> 24);
		out[4 * i + 1] = (uint8_t)(state[i] >> 16);
		out[4 * i + 2] = (uint8_t)(state[i] >> 8);
		out[4 * i + 3] = (uint8_t)state[i];
	}
}

void sha256_hash(const uint8_t* data, size_t len, uint8_t out[32]) {
	uint32_t state[8];
	memcpy(state, kSha256Init, sizeof(state));
	size_t at = 0;
	for (; at + 64 <= len; at += 64) sha256_compress(state, data + at);
	uint8_t last[128] = {0};
	const size_t rest = len - at;
	if (rest) memcpy(last, data + at, rest);
	last[rest] = 0x80;
	const size_t n = rest + 9 <= 64 ? 64 : 128;
	const uint64_t bits = (uint64_t)len * 8;
	for (int i = 0; i < 8; i++) last[n - 1 - i] = (uint8_t)(bits >> (8 * i));
	sha256_compress(state, last);
	if (n == 128) sha256_compress(state, last + 64);
	put_state(state, out);
}

void mk_hash_leaf(const uint8_t* leaf, int log_leaf_elems, uint8_t out[32]) { sha256_hash(leaf, (size_t)16 << log_leaf_elems, out); }

void mk_hash_node(const uint8_t left[32], const uint8_t right[32], uint8_t out[32]) {
	uint8_t block[64];
	memcpy(block, left, 32);
	memcpy(block + 32, right, 32);
	uint32_t state[8];
	memcpy(state, kSha256Init, sizeof(state));
	sha256_compress(state, block);
	put_state(state, out);
}

bool mk_verify(const uint8_t root[32], int log_leaves, int log_leaf_elems, uint64_t index, const uint8_t* record) {
	if (index >> log_leaves) return false;
	uint8_t cur[32], nxt[32];
	mk_hash_leaf(record, log_leaf_elems, cur);
	const uint8_t* sib = record + ((size_t)16 << log_leaf_elems);
	for (int h = 0; h < log_leaves; h++, sib += 32) {
		if ((index >> h) & 1)
			mk_hash_node(sib, cur, nxt);
		else
			mk_hash_node(cur, sib, nxt);
		memcpy(cur, nxt, 32);
	}
	return memcmp(cur, root, 32) == 0;
}

}  // namespace bn
