// The SHA-256 Merkle commitment of a GF(2^128) codeword over the C-ABI, on __uint128_t values (4
// little-endian u32 limbs, bigints.cu:6-13). No reference counterpart. Header-only.
//
// Leaf j is the 2^log_leaf_elems consecutive elements [j << a, (j + 1) << a); its digest is the padded
// SHA-256 of its bytes, a node's digest one compression of left || right from the initial state. The
// tree is 2^(L+1) - 1 digests, row 0 (the leaf digests) first and the root last; an opening record is
// the leaf's bytes and then the L sibling digests from the bottom up (include/binius_ntt_amd.h).
#pragma once

#include <array>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "../utils/common.hpp"

typedef std::array<uint8_t, 32> MerkleDigest;

// 2^(log_leaves + 1) - 1: the digests of the tree buffer
inline size_t merkle_tree_digests(int log_leaves) {
	size_t n = 0;
	ulvt::bn_check(bn_merkle_tree_digests(log_leaves, &n));
	return n;
}

// digest index of node 0 of `row` (row 0: the leaf digests, row log_leaves: the root)
inline size_t merkle_row_offset(int log_leaves, int row) {
	size_t at = 0;
	ulvt::bn_check(bn_merkle_row_offset(log_leaves, row, &at));
	return at;
}

// bytes of one opening record
inline size_t merkle_open_bytes(int log_leaves, int log_leaf_elems) {
	size_t n = 0;
	ulvt::bn_check(bn_merkle_open_bytes(log_leaves, log_leaf_elems, &n));
	return n;
}

// The tree of a host codeword of 2^(L + a) elements, computed on the GPU (synchronous).
// std::invalid_argument unless the size is a power of two of at least one leaf.
inline std::vector<MerkleDigest> merkle_commit(const std::vector<__uint128_t>& data, int log_leaf_elems, int device = 0) {
	int log_n = 0;
	while (((size_t)1 << log_n) < data.size()) log_n++;
	if (data.empty() || ((size_t)1 << log_n) != data.size() || log_leaf_elems < 0 || log_leaf_elems > log_n)
		throw std::invalid_argument("merkle_commit: the data must hold a power of two of elements, at least one leaf");
	const int log_leaves = log_n - log_leaf_elems;
	std::vector<MerkleDigest> tree(((size_t)2 << log_leaves) - 1);
	ulvt::bn_check(bn_merkle_commit_host(device, (const uint32_t*)data.data(), log_leaves, log_leaf_elems, tree[0].data()));
	return tree;
}

// The same from device memory into device memory (32 * merkle_tree_digests bytes), asynchronous on
// `stream` (a hipStream_t, may be null); d_data is left untouched.
inline void merkle_commit_device(const void* d_data, int log_leaves, int log_leaf_elems, void* d_tree, void* stream = nullptr) {
	ulvt::bn_check(bn_merkle_commit_device(d_data, log_leaves, log_leaf_elems, d_tree, stream));
}

// Opening records of the leaves d_indices[0 .. n_queries) (device memory, uint32) at
// d_out + q * merkle_open_bytes, asynchronous on `stream`; an index >= 2^L gives an all-zero record.
inline void merkle_open_device(const void* d_data, const void* d_tree, int log_leaves, int log_leaf_elems,
                               const uint32_t* d_indices, size_t n_queries, void* d_out, void* stream = nullptr) {
	ulvt::bn_check(bn_merkle_open_device(d_data, d_tree, log_leaves, log_leaf_elems, d_indices, n_queries, d_out, stream));
}

// True if `record` opens leaf `index` of the tree with this root (host arithmetic).
// std::invalid_argument if the record's size is not merkle_open_bytes.
inline bool merkle_verify(const MerkleDigest& root, int log_leaves, int log_leaf_elems, uint64_t index,
                          const std::vector<uint8_t>& record) {
	if (record.size() != merkle_open_bytes(log_leaves, log_leaf_elems))
		throw std::invalid_argument("merkle_verify: the record's size is not that of an opening");
	int ok = 0;
	ulvt::bn_check(bn_merkle_verify(root.data(), log_leaves, log_leaf_elems, index, record.data(), &ok));
	return ok == 1;
}
