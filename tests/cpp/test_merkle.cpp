// The Merkle commitment of the C++ mirror (binius-ntt_amd/host/ulvt/merkle/merkle_tree.hpp), built
// against the C-ABI alone. There is no reference counterpart: the tree the GPU computes is compared
// with one built from the host-only bn_merkle_hash_leaf / bn_merkle_hash_node calls, records put
// together from it are checked with merkle_verify, and the argument errors are raised.
#include <cstdio>
#include <cstring>
#include <vector>

#include "merkle/merkle_tree.hpp"
#include "../../oracle/oracle.h"

typedef unsigned __int128 u128;

static int failures = 0;
static void check(bool ok, const char* what) {
	std::printf("%s %s\n", ok ? "ok" : "FAIL", what);
	if (!ok) failures++;
}

static std::vector<MerkleDigest> host_tree(const std::vector<u128>& data, int L, int a) {
	std::vector<MerkleDigest> tree(merkle_tree_digests(L));
	for (size_t j = 0; j < ((size_t)1 << L); j++) ulvt::bn_check(bn_merkle_hash_leaf(&data[j << a], a, tree[j].data()));
	for (int h = 1; h <= L; h++) {
		const size_t from = merkle_row_offset(L, h - 1), to = merkle_row_offset(L, h);
		for (size_t k = 0; k < ((size_t)1 << (L - h)); k++)
			ulvt::bn_check(bn_merkle_hash_node(tree[from + 2 * k].data(), tree[from + 2 * k + 1].data(), tree[to + k].data()));
	}
	return tree;
}

static void flow(int L, int a) {
	std::vector<u128> data((size_t)1 << (L + a));
	orc_fill128(0x3e4b0000 + 16 * L + a, 0xc0ffee00, (uint32_t*)data.data(), data.size());
	char what[128];
	const std::vector<MerkleDigest> got = merkle_commit(data, a);
	const std::vector<MerkleDigest> want = host_tree(data, L, a);
	std::snprintf(what, sizeof(what), "merkle_commit L=%d a=%d equals the tree of the host hashes", L, a);
	check(got.size() == merkle_tree_digests(L) && got == want, what);
	std::snprintf(what, sizeof(what), "L=%d: the rows are consecutive and the root is last", L);
	check(merkle_row_offset(L, 0) == 0 && merkle_row_offset(L, L) == got.size() - 1 &&
	          (L == 0 || merkle_row_offset(L, 1) == ((size_t)1 << L)),
	      what);
	bool ok = true, rejected = true;
	for (size_t j : {(size_t)0, ((size_t)1 << L) - 1, (size_t)0x1b35 & (((size_t)1 << L) - 1)}) {
		std::vector<uint8_t> rec(merkle_open_bytes(L, a));
		std::memcpy(rec.data(), &data[j << a], (size_t)16 << a);
		for (int h = 0; h < L; h++) std::memcpy(&rec[((size_t)16 << a) + 32 * h], got[merkle_row_offset(L, h) + ((j >> h) ^ 1)].data(), 32);
		ok = ok && merkle_verify(got.back(), L, a, j, rec);
		rejected = rejected && !merkle_verify(got.back(), L, a, j ^ 1, rec);
		rec[rec.size() / 2] ^= 1;
		rejected = rejected && !merkle_verify(got.back(), L, a, j, rec);
	}
	std::snprintf(what, sizeof(what), "merkle_verify L=%d a=%d accepts records of the GPU's tree, rejects tampered ones", L, a);
	check(ok && rejected, what);
}

template <class F>
static bool throws_invalid(F f) {
	try {
		f();
	} catch (const ulvt::BnError& e) {
		return e.code == BN_ERR_INVALID;
	} catch (const std::invalid_argument&) {
		return true;
	}
	return false;
}

static void rejects() {
	std::vector<u128> data(16, 7);
	char fake[64];  // never dereferenced: the calls fail their checks first
	void* const p = (void*)(((uintptr_t)fake + 15) & ~(uintptr_t)15);
	check(throws_invalid([&] { merkle_commit(std::vector<u128>(12, 1), 2); }), "merkle_commit rejects 12 elements");
	check(throws_invalid([&] { merkle_commit(data, 5); }), "merkle_commit rejects a leaf larger than the data");
	check(throws_invalid([&] { merkle_commit_device(nullptr, 2, 2, p); }), "merkle_commit_device rejects a NULL buffer");
	check(throws_invalid([&] { merkle_commit_device(p, 2, 9, (char*)p + (1 << 20)); }), "merkle_commit_device rejects log_leaf_elems = 9");
	check(throws_invalid([&] { merkle_commit_device(p, 2, 2, p); }), "merkle_commit_device rejects overlapping buffers");
	check(throws_invalid([&] { merkle_open_device(p, (char*)p + (1 << 20), 2, 2, (const uint32_t*)((char*)p + (2 << 20)), 0, (char*)p + (3 << 20)); }),
	      "merkle_open_device rejects no query");
	check(throws_invalid([&] { merkle_verify(MerkleDigest{}, 2, 2, 0, std::vector<uint8_t>(10)); }), "merkle_verify rejects a short record");
	check(throws_invalid([&] { merkle_tree_digests(31); }) && throws_invalid([&] { merkle_row_offset(4, 5); }),
	      "the sizes reject a tree of 2^31 leaves and a row above the root");
	const std::vector<MerkleDigest> got = merkle_commit(data, 2);
	check(got == host_tree(data, 2, 2), "merkle_commit works after the rejected calls");
}

int main() {
	flow(7, 4);
	flow(13, 2);
	rejects();
	std::printf("%s (%d failures)\n", failures ? "FAILED" : "PASSED", failures);
	return failures ? 1 : 0;
}
