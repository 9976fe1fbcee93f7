// Pass planning of the SHA-256 Merkle commitment (host only, merkle_plan.cpp): how the L + 1 rows of
// the tree are split into passes, where a row lies in the tree buffer, which nodes a work-group
// writes, the LDS sizes and the grid rule; and a plain C++ SHA-256 (compression and padded hash) for
// the verifier's host-only calls. No HIP header: this is integer code, and the device side
// (merkle.hip, sha256_dev.hpp) includes this file for the constants and the address functions, so the
// kernels and the host-side sweep (tests/cpp/test_merkle_plan.cpp) use the same ones.
//
// The tree buffer holds 2^(L+1) - 1 digests of 32 bytes: row 0 (the 2^L leaf digests) first, row h
// (2^(L-h) nodes) at digest index 2^(L+1) - 2^(L-h+1), the root last. Node k of row h + 1 is
// node(row_h[2k], row_h[2k+1]).
//
// Passes. The leaf pass hashes 256 leaves a work-group (row 0) and, when every work-group is full
// (L >= 8), goes on to rows 1 and 2 (128 and 64 nodes a work-group: whole waves). A row pass takes
// 512 consecutive digests of row h a work-group and writes rows h+1 .. h+3 (256, 128, 64 nodes).
// The tail is the row kernel on one work-group: it starts from a row of at most 2^9 digests and
// writes every row up to the root. A forced cap m (1 .. 3, the test hook) limits every pass, the
// tail included, to m rows, so that small trees have row passes and a short tail; a row pass then
// also takes rows of fewer than 512 digests (one work-group, partly filled).
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace bn {

constexpr int kMkMaxLogElems = 30;     // L + a
constexpr int kMkMaxLeafLog = 8;       // a: a leaf of up to 256 elements (4 KiB, 65 blocks)
constexpr int kMkThreads = 256;        // work-group of every kernel
constexpr int kMkLeafGroupLog = 8;     // leaves of a work-group of the leaf pass
constexpr int kMkRowGroupLog = 9;      // child digests of a work-group of a row pass
constexpr int kMkRowsPerPass = 3;      // rows a leaf or row pass writes: down to one full wave
constexpr int kMkTailRows = kMkRowGroupLog;  // rows the tail writes by default: from <= 2^9 digests
constexpr int kMkMaxPasses = 32;       // room for leaf + 29 one-row passes + tail (L = 30, cap 1)

enum MkKind { kMkLeaf = 0, kMkRow = 1, kMkTail = 2 };

struct MkPass {
	int kind;       // MkKind
	int first_row;  // the first row written
	int rows;       // rows written: first_row .. first_row + rows - 1
};
struct MkPlan {
	int n_passes;
	MkPass pass[kMkMaxPasses];
};

// The split of rows 0 .. log_leaves at the cap max_rows (0: the default, kMkRowsPerPass for the leaf
// and row passes and kMkTailRows for the tail; m in [1, kMkRowsPerPass]: m for every pass). One leaf
// pass first; the tail, if there are rows left, last with min(tail cap, rows left) rows; the rows
// between them in row passes of cap rows, the first taking the remainder. False, with *plan
// untouched, unless 0 <= log_leaf_elems <= 8, 0 <= log_leaves, log_leaves + log_leaf_elems <= 30 and
// 0 <= max_rows <= kMkRowsPerPass.
bool mk_plan(int log_leaves, int log_leaf_elems, int max_rows, MkPlan* plan);

constexpr uint64_t mk_tree_digests(int log_leaves) { return ((uint64_t)2 << log_leaves) - 1; }
constexpr uint64_t mk_row_nodes(int log_leaves, int row) { return (uint64_t)1 << (log_leaves - row); }
// digest index of node 0 of `row`
constexpr uint64_t mk_row_offset(int log_leaves, int row) { return ((uint64_t)2 << log_leaves) - ((uint64_t)2 << (log_leaves - row)); }
constexpr uint64_t mk_open_bytes(int log_leaves, int log_leaf_elems) { return ((uint64_t)16 << log_leaf_elems) + 32 * (uint64_t)log_leaves; }

// A work-group's share of a pass. group_log is kMkLeafGroupLog (leaf pass: leaves) or kMkRowGroupLog
// (row pass, tail: digests of the row read); a row shorter than a group is one partly filled group.
constexpr uint64_t mk_groups(int log_leaves, int row_in, int group_log) {
	return log_leaves - row_in > group_log ? (uint64_t)1 << (log_leaves - row_in - group_log) : 1;
}
// items (leaves or digests read) of one group
constexpr uint32_t mk_group_items(int log_leaves, int row_in, int group_log) {
	return (uint32_t)1 << (log_leaves - row_in > group_log ? group_log : log_leaves - row_in);
}
// nodes a group writes into row row_in + k (k >= 1), and the first of them (node index in that row)
constexpr uint32_t mk_group_nodes(int log_leaves, int row_in, int group_log, int k) { return mk_group_items(log_leaves, row_in, group_log) >> k; }
constexpr uint64_t mk_group_first_node(int log_leaves, int row_in, int group_log, int k, uint64_t group) {
	return group * mk_group_nodes(log_leaves, row_in, group_log, k);
}

// LDS. Digests between the rows of a pass lie as eight word planes of `cap` entries each, a plane
// cap + 8 words long: a lane reads its two children as one 8-byte access per plane (stride 2
// words: no bank conflict), and the two halves of a digest loaded by neighbouring lanes fall 32
// banks apart. The leaf pass first stages a wave's 64 leaves, up to 128 bytes of each at a time, in
// rows padded by 16 bytes (so that the lanes' 16-byte reads of their own rows spread over all banks).
constexpr uint32_t mk_plane_words(uint32_t cap) { return cap + 8; }
constexpr uint32_t mk_digest_lds_words(uint32_t cap) { return 8 * (mk_plane_words(cap) + mk_plane_words(cap / 2)); }
constexpr int mk_chunk_vecs(int log_leaf_elems) { return log_leaf_elems < 3 ? 1 << log_leaf_elems : 8; }  // 16-byte vectors of a leaf staged at a time
constexpr uint32_t mk_stage_row_words(int log_leaf_elems) { return 4 * mk_chunk_vecs(log_leaf_elems) + (log_leaf_elems ? 4 : 0); }
constexpr uint32_t mk_leaf_lds_words(int log_leaf_elems) {
	const uint32_t stage = kMkThreads * mk_stage_row_words(log_leaf_elems), dig = mk_digest_lds_words(1u << kMkLeafGroupLog);
	return stage > dig ? stage : dig;
}
constexpr uint32_t mk_row_lds_words() { return mk_digest_lds_words(1u << kMkRowGroupLog); }
constexpr size_t kMkLdsPerGroup = 64 * 1024;  // static LDS of a kernel

// ---- SHA-256 (FIPS 180-4)
constexpr uint32_t kSha256Init[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
constexpr uint32_t kSha256K[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
    0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
    0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
    0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
    0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
    0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

// state <- compression of the 64-byte block (big-endian words), feed-forward included
void sha256_compress(uint32_t state[8], const uint8_t block[64]);
// the padded hash of len bytes; out: 32 bytes, big-endian state words
void sha256_hash(const uint8_t* data, size_t len, uint8_t out[32]);
// digest of a leaf of 2^log_leaf_elems elements: sha256_hash of its 16 << log_leaf_elems bytes
void mk_hash_leaf(const uint8_t* leaf, int log_leaf_elems, uint8_t out[32]);
// digest of a node: one compression of left || right from the initial state, no padding
void mk_hash_node(const uint8_t left[32], const uint8_t right[32], uint8_t out[32]);
// an opening record (the leaf's bytes, then log_leaves sibling digests from the bottom up) against a root
bool mk_verify(const uint8_t root[32], int log_leaves, int log_leaf_elems, uint64_t index, const uint8_t* record);

}  // namespace bn
