// SHA-256 Merkle commitment of a device-resident GF(2^128) codeword, and its query openings. No
// reference counterpart.
//
// Rule (include/binius_ntt_amd.h has it in full): leaf j is the 2^a consecutive elements
// [j << a, (j + 1) << a) as they lie in memory; its digest is the padded SHA-256 of those bytes. A
// node's digest is one compression of left || right from the initial state. The tree buffer holds row
// 0 (the leaf digests) first and the root last (merkle_plan.hpp: mk_row_offset).
//
// Passes (merkle_plan.hpp plans them; stream order between the launches is the only synchronisation,
// every pass reads the row the one before it wrote into d_tree; nothing is allocated):
//
//   merkle_leaf_pass<A>  one lane hashes one leaf, 256 leaves a work-group. A wave's 64 leaves are one
//                        contiguous run; it is moved with coalesced non-temporal 16-byte loads, up to
//                        128 bytes of every leaf at a time, through padded LDS rows, from which each
//                        lane reads its own leaf's blocks (the next chunk's loads are in flight while
//                        the lane compresses). A limb becomes a message word by one byte permute. For
//                        a >= 2 the last block is nothing but padding: its schedule plus the round
//                        constants are 64 literals and the block runs rounds only; for a <= 1 the one
//                        block is data and constants. The pass then goes on to rows 1 and 2 (128 and 64
//                        nodes on whole waves), the digests passing through LDS word planes.
//   merkle_row_pass      a work-group loads 512 consecutive digests of row h and writes rows h+1 ..
//                        h+3 (256, 128, 64 nodes) the same way. Launched as one work-group with up
//                        to nine rows it is the tail: every remaining row up to the root, a barrier
//                        between rows instead of a launch.
//   merkle_open          one 64-lane work-group a query copies the leaf and gathers the siblings.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "merkle_plan.hpp"
#include "sha256_dev.hpp"
#include "stream_io.hpp"

namespace bn {

static_assert(kMkThreads == 1 << kMkLeafGroupLog, "one lane a leaf");
static_assert(2 * kMkThreads == 1 << kMkRowGroupLog, "one lane a node of the first row written");
static_assert(kMkThreads >> (kMkRowsPerPass - 1) >= 64, "a fused row fills a wave");
static_assert(mk_leaf_lds_words(kMkMaxLeafLog) * 4 <= kMkLdsPerGroup && mk_row_lds_words() * 4 <= kMkLdsPerGroup, "static LDS");

__device__ __forceinline__ uint32_t mk_bswap(uint32_t x) { return __builtin_bswap32(x); }
__device__ __forceinline__ uint4 mk_bswap4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
	return make_uint4(mk_bswap(a), mk_bswap(b), mk_bswap(c), mk_bswap(d));
}

__device__ __forceinline__ void mk_store_digest(uint4* tree, uint64_t index, const uint32_t (&st)[8]) {
	tree[2 * index] = mk_bswap4(st[0], st[1], st[2], st[3]);
	tree[2 * index + 1] = mk_bswap4(st[4], st[5], st[6], st[7]);
}

// The group's digests of row row_in lie in `cur` (eight word planes of stride cs, state words as
// they are); writes rows row_in + 1 .. row_in + rows to the tree, the planes alternating between cur
// and nxt. Every thread of the work-group calls it.
__device__ __forceinline__ void mk_node_rows(uint32_t* cur, uint32_t cs, uint32_t* nxt, uint32_t ns, uint4* tree, int log_leaves,
                                             int row_in, int group_log, int rows) {
	const uint32_t tid = threadIdx.x;
#pragma unroll 1
	for (int k = 1; k <= rows; k++) {
		const uint32_t n = mk_group_nodes(log_leaves, row_in, group_log, k);
		if (tid < n) {
			uint32_t w[16], st[8];
#pragma unroll
			for (int p = 0; p < 8; p++) {
				const uint2 c = *(const uint2*)(cur + p * cs + 2 * tid);
				w[p] = c.x;
				w[8 + p] = c.y;
			}
			sha256_init(st);
			sha256_block(st, w);
			if (k < rows) {
#pragma unroll
				for (int p = 0; p < 8; p++) nxt[p * ns + tid] = st[p];
			}
			mk_store_digest(tree, mk_row_offset(log_leaves, row_in + k) + mk_group_first_node(log_leaves, row_in, group_log, k, blockIdx.x) + tid,
			                st);
		}
		__syncthreads();
		uint32_t* const t = cur;
		cur = nxt;
		nxt = t;
		const uint32_t ts = cs;
		cs = ns;
		ns = ts;
	}
}

struct MkLeafParams {
	const uint4* data;
	uint4* tree;
	int log_leaves;
	int rows;  // rows written: 1 + the fused ones
};

template <int A>
__global__ __launch_bounds__(kMkThreads) void merkle_leaf_pass(MkLeafParams P) {
	constexpr int E = 1 << A;              // 16-byte vectors of a leaf
	constexpr int C4 = mk_chunk_vecs(A);   // of them, staged at a time
	constexpr int NCH = E / C4;
	constexpr uint32_t RS = mk_stage_row_words(A);
	__shared__ uint4 lds4[mk_leaf_lds_words(A) / 4];
	uint32_t* const lds = (uint32_t*)lds4;
	const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	uint32_t* const stage = lds + wave * 64 * RS;  // the wave's 64 rows
	const uint64_t n_leaves = (uint64_t)1 << P.log_leaves;
	const uint64_t wave_leaf = (uint64_t)blockIdx.x * kMkThreads + wave * 64;

	uint4 g[C4];
	auto load = [&](int ch) {
#pragma unroll
		for (int i = 0; i < C4; i++) {
			const uint32_t x = i * 64 + lane;  // consecutive lanes, consecutive 16 bytes of the run
			const uint64_t leaf = wave_leaf + x / C4;
			// streaming: the codeword is read once
			g[i] = leaf < n_leaves ? ld_stream((const uint32_t*)(P.data + leaf * E + (uint64_t)ch * C4 + x % C4)) : make_uint4(0, 0, 0, 0);
		}
	};

	uint32_t st[8];
	sha256_init(st);
	load(0);
#pragma unroll 1
	for (int ch = 0; ch < NCH; ch++) {
		if (ch) __syncthreads();  // the chunk before has been read
#pragma unroll
		for (int i = 0; i < C4; i++) {
			const uint32_t x = i * 64 + lane;
			*(uint4*)(stage + (x / C4) * RS + 4 * (x % C4)) = g[i];
		}
		__syncthreads();
		if (ch + 1 < NCH) load(ch + 1);
		const uint32_t* const row = stage + lane * RS;
		uint32_t w[16];
		if constexpr (A >= 2) {
#pragma unroll 1
			for (int blk = 0; blk < C4 / 4; blk++) {
#pragma unroll
				for (int q = 0; q < 4; q++) {
					const uint4 v = *(const uint4*)(row + 16 * blk + 4 * q);
					w[4 * q] = mk_bswap(v.x), w[4 * q + 1] = mk_bswap(v.y), w[4 * q + 2] = mk_bswap(v.z), w[4 * q + 3] = mk_bswap(v.w);
				}
				sha256_block(st, w);
			}
		} else {
			// data and padding in one block
#pragma unroll
			for (int q = 0; q < 4; q++) {
				uint4 v = make_uint4(0, 0, 0, 0);
				if (q < E) v = *(const uint4*)(row + 4 * q);
				w[4 * q] = mk_bswap(v.x), w[4 * q + 1] = mk_bswap(v.y), w[4 * q + 2] = mk_bswap(v.z), w[4 * q + 3] = mk_bswap(v.w);
			}
			w[4 * E] = 0x80000000u;
			w[15] = 128 * E;  // bits
			sha256_block(st, w);
		}
	}
	if constexpr (A >= 2) sha256_pad_block<16u * E>(st);

	__syncthreads();  // the stage is read no more: the digest planes take its place
	constexpr uint32_t cs = mk_plane_words(kMkThreads), ns = mk_plane_words(kMkThreads / 2);
	uint32_t* const cur = lds;
	uint32_t* const nxt = lds + 8 * cs;
	if (P.rows > 1) {
#pragma unroll
		for (int p = 0; p < 8; p++) cur[p * cs + tid] = st[p];
	}
	const uint64_t leaf = (uint64_t)blockIdx.x * kMkThreads + tid;
	if (leaf < n_leaves) mk_store_digest(P.tree, leaf, st);
	__syncthreads();
	mk_node_rows(cur, cs, nxt, ns, P.tree, P.log_leaves, 0, kMkLeafGroupLog, P.rows - 1);
}

struct MkRowParams {
	uint4* tree;
	int log_leaves;
	int row_in;  // the row read
	int rows;    // rows written: row_in + 1 .. row_in + rows
};

__global__ __launch_bounds__(kMkThreads) void merkle_row_pass(MkRowParams P) {
	__shared__ uint4 lds4[mk_row_lds_words() / 4];
	uint32_t* const lds = (uint32_t*)lds4;
	constexpr uint32_t cs = mk_plane_words(1u << kMkRowGroupLog), ns = mk_plane_words(1u << (kMkRowGroupLog - 1));
	const uint32_t tid = threadIdx.x;
	const uint32_t items = mk_group_items(P.log_leaves, P.row_in, kMkRowGroupLog);
	const uint4* const src = P.tree + 2 * (mk_row_offset(P.log_leaves, P.row_in) + (uint64_t)blockIdx.x * items);
#pragma unroll
	for (int i = 0; i < (2 << kMkRowGroupLog) / kMkThreads; i++) {
		const uint32_t x = tid + i * kMkThreads;  // 16-byte half x & 1 of digest x >> 1
		if (x < 2 * items) {
			const uint4 v = src[x];
			uint32_t* const d = lds + (x & 1) * 4 * cs + (x >> 1);
			d[0] = mk_bswap(v.x), d[cs] = mk_bswap(v.y), d[2 * cs] = mk_bswap(v.z), d[3 * cs] = mk_bswap(v.w);
		}
	}
	__syncthreads();
	mk_node_rows(lds, cs, lds + 8 * cs, ns, P.tree, P.log_leaves, P.row_in, kMkRowGroupLog, P.rows);
}

struct MkOpenParams {
	const uint4* data;
	const uint4* tree;
	const uint32_t* indices;
	uint4* out;
	unsigned long long n_queries;
	int log_leaves;
	int log_leaf_elems;
};

constexpr int kMkOpenThreads = 64;

__global__ __launch_bounds__(kMkOpenThreads) void merkle_open(MkOpenParams P) {
	const uint32_t leaf_vecs = 1u << P.log_leaf_elems, vecs = leaf_vecs + 2 * P.log_leaves;
	for (unsigned long long q = blockIdx.x; q < P.n_queries; q += gridDim.x) {
		const uint64_t j = P.indices[q];
		const bool in_range = j < ((uint64_t)1 << P.log_leaves);
		uint4* const rec = P.out + q * vecs;
		for (uint32_t x = threadIdx.x; x < vecs; x += kMkOpenThreads) {
			uint4 v = make_uint4(0, 0, 0, 0);
			if (in_range) {
				if (x < leaf_vecs) {
					v = P.data[(j << P.log_leaf_elems) + x];
				} else {
					const int h = (x - leaf_vecs) >> 1;  // the sibling at row h
					v = P.tree[2 * (mk_row_offset(P.log_leaves, h) + ((j >> h) ^ 1)) + ((x - leaf_vecs) & 1)];
				}
			}
			rec[x] = v;
		}
	}
}

template <int A>
static int mk_launch_leaf(const MkLeafParams& prm, unsigned grid, hipStream_t st) {
	MkLeafParams p = prm;
	void* args[] = {&p};
	BN_HIP(hipLaunchKernel((const void*)merkle_leaf_pass<A>, dim3(grid), dim3(kMkThreads), args, 0, st));
	return BN_OK;
}

// Every pass of the plan on `st`. Arguments are checked by the caller; the current device is the buffers'.
static int mk_launch(const MkPlan& plan, const void* d_data, int log_leaves, int log_leaf_elems, void* d_tree, hipStream_t st) {
	for (int i = 0; i < plan.n_passes; i++) {
		const MkPass& ps = plan.pass[i];
		if (ps.kind == kMkLeaf) {
			const MkLeafParams prm{(const uint4*)d_data, (uint4*)d_tree, log_leaves, ps.rows};
			const unsigned grid = (unsigned)mk_groups(log_leaves, 0, kMkLeafGroupLog);
			int rc = BN_OK;
			switch (log_leaf_elems) {
				case 0: rc = mk_launch_leaf<0>(prm, grid, st); break;
				case 1: rc = mk_launch_leaf<1>(prm, grid, st); break;
				case 2: rc = mk_launch_leaf<2>(prm, grid, st); break;
				case 3: rc = mk_launch_leaf<3>(prm, grid, st); break;
				case 4: rc = mk_launch_leaf<4>(prm, grid, st); break;
				case 5: rc = mk_launch_leaf<5>(prm, grid, st); break;
				case 6: rc = mk_launch_leaf<6>(prm, grid, st); break;
				case 7: rc = mk_launch_leaf<7>(prm, grid, st); break;
				default: rc = mk_launch_leaf<8>(prm, grid, st); break;
			}
			if (rc != BN_OK) return rc;
		} else {
			MkRowParams prm{(uint4*)d_tree, log_leaves, ps.first_row - 1, ps.rows};
			const unsigned grid = (unsigned)mk_groups(log_leaves, prm.row_in, kMkRowGroupLog);
			void* args[] = {&prm};
			BN_HIP(hipLaunchKernel((const void*)merkle_row_pass, dim3(grid), dim3(kMkThreads), args, 0, st));
		}
	}
	return BN_OK;
}

static int mk_check_shape(int log_leaves, int log_leaf_elems) {
	BN_CHECK_ARG(log_leaf_elems >= 0 && log_leaf_elems <= kMkMaxLeafLog, "log_leaf_elems must be in [0, %d] (got %d)", kMkMaxLeafLog,
	             log_leaf_elems);
	BN_CHECK_ARG(log_leaves >= 0 && log_leaves + log_leaf_elems <= kMkMaxLogElems,
	             "log_leaves must be >= 0 and log_leaves + log_leaf_elems <= %d (got %d + %d)", kMkMaxLogElems, log_leaves, log_leaf_elems);
	return BN_OK;
}

// `device`: the buffers are device memory, accessed 16 bytes at a time
static int mk_check_commit(const void* data, int log_leaves, int log_leaf_elems, const void* tree, int max_rows, bool device, MkPlan* plan) {
	BN_CHECK_ARG(data != nullptr && tree != nullptr, "NULL buffer");
	if (int rc = mk_check_shape(log_leaves, log_leaf_elems)) return rc;
	BN_CHECK_ARG(mk_plan(log_leaves, log_leaf_elems, max_rows, plan), "max_rows must be in [0, %d] (got %d)", kMkRowsPerPass, max_rows);
	BN_CHECK_ARG(!device || (is_aligned(data, 16) && is_aligned(tree, 16)), "the buffers must be 16-byte aligned");
	BN_CHECK_ARG(!ranges_overlap(data, (uint64_t)16 << (log_leaves + log_leaf_elems), tree, 32 * mk_tree_digests(log_leaves)),
	             "the data and the tree overlap");
	return BN_OK;
}

}  // namespace bn

using namespace bn;

extern "C" int bn_merkle_tree_digests(int log_leaves, size_t* n) {
	BN_CHECK_ARG(n != nullptr, "NULL argument");
	BN_CHECK_ARG(log_leaves >= 0 && log_leaves <= kMkMaxLogElems, "log_leaves must be in [0, %d] (got %d)", kMkMaxLogElems, log_leaves);
	*n = (size_t)mk_tree_digests(log_leaves);
	return BN_OK;
}

extern "C" int bn_merkle_row_offset(int log_leaves, int row, size_t* index) {
	BN_CHECK_ARG(index != nullptr, "NULL argument");
	BN_CHECK_ARG(log_leaves >= 0 && log_leaves <= kMkMaxLogElems, "log_leaves must be in [0, %d] (got %d)", kMkMaxLogElems, log_leaves);
	BN_CHECK_ARG(row >= 0 && row <= log_leaves, "row must be in [0, %d] (got %d)", log_leaves, row);
	*index = (size_t)mk_row_offset(log_leaves, row);
	return BN_OK;
}

extern "C" int bn_merkle_open_bytes(int log_leaves, int log_leaf_elems, size_t* bytes) {
	BN_CHECK_ARG(bytes != nullptr, "NULL argument");
	if (int rc = mk_check_shape(log_leaves, log_leaf_elems)) return rc;
	*bytes = (size_t)mk_open_bytes(log_leaves, log_leaf_elems);
	return BN_OK;
}

extern "C" int bn_merkle_commit_device_split(const void* d_data, int log_leaves, int log_leaf_elems, void* d_tree, int max_rows,
                                             void* stream) {
	MkPlan plan;
	if (int rc = mk_check_commit(d_data, log_leaves, log_leaf_elems, d_tree, max_rows, true, &plan)) return rc;
	return mk_launch(plan, d_data, log_leaves, log_leaf_elems, d_tree, (hipStream_t)stream);
}

extern "C" int bn_merkle_commit_device(const void* d_data, int log_leaves, int log_leaf_elems, void* d_tree, void* stream) {
	return bn_merkle_commit_device_split(d_data, log_leaves, log_leaf_elems, d_tree, 0, stream);
}

extern "C" int bn_merkle_commit_host(int device, const uint32_t* data, int log_leaves, int log_leaf_elems, uint8_t* tree) {
	MkPlan plan;
	if (int rc = mk_check_commit(data, log_leaves, log_leaf_elems, tree, 0, false, &plan)) return rc;
	BN_DEVICE_SCOPE(device);
	const size_t data_bytes = (size_t)16 << (log_leaves + log_leaf_elems), tree_bytes = (size_t)(32 * mk_tree_digests(log_leaves));
	// staged per call, data and tree in one allocation (both sizes are multiples of 16)
	DevBuf buf;
	CallStream cs;
	if (int rc = buf.alloc(data_bytes + tree_bytes)) return rc;
	if (int rc = cs.create()) return rc;
	void* d_tree = (uint8_t*)buf.p + data_bytes;
	return staged_call(cs.s, data, buf.p, data_bytes, d_tree, tree, tree_bytes,
	                   [&](hipStream_t st) { return mk_launch(plan, buf.p, log_leaves, log_leaf_elems, d_tree, st); });
}

extern "C" int bn_merkle_open_device(const void* d_data, const void* d_tree, int log_leaves, int log_leaf_elems, const uint32_t* d_indices,
                                     size_t n_queries, void* d_out, void* stream) {
	BN_CHECK_ARG(d_data != nullptr && d_tree != nullptr && d_indices != nullptr && d_out != nullptr, "NULL buffer");
	if (int rc = mk_check_shape(log_leaves, log_leaf_elems)) return rc;
	const uint64_t rec = mk_open_bytes(log_leaves, log_leaf_elems);
	BN_CHECK_ARG(n_queries >= 1 && n_queries <= ((uint64_t)1 << 40) / rec, "n_queries must be in [1, 2^40 / record bytes] (got %zu)", n_queries);
	BN_CHECK_ARG(is_aligned(d_data, 16) && is_aligned(d_tree, 16) && is_aligned(d_out, 16) && is_aligned(d_indices, 4),
	             "the buffers must be 16-byte aligned, the indices 4-byte");
	const uint64_t data_bytes = (uint64_t)16 << (log_leaves + log_leaf_elems), tree_bytes = 32 * mk_tree_digests(log_leaves);
	BN_CHECK_ARG(!ranges_overlap(d_data, data_bytes, d_tree, tree_bytes), "the data and the tree overlap");
	BN_CHECK_ARG(!ranges_overlap(d_out, n_queries * rec, d_data, data_bytes) && !ranges_overlap(d_out, n_queries * rec, d_tree, tree_bytes) &&
	                 !ranges_overlap(d_out, n_queries * rec, d_indices, 4 * (uint64_t)n_queries),
	             "the output overlaps the data, the tree or the indices");
	MkOpenParams prm{(const uint4*)d_data, (const uint4*)d_tree, d_indices, (uint4*)d_out, (unsigned long long)n_queries, log_leaves, log_leaf_elems};
	const unsigned grid = (unsigned)(n_queries < (1u << 20) ? n_queries : (1u << 20));
	void* args[] = {&prm};
	BN_HIP(hipLaunchKernel((const void*)merkle_open, dim3(grid), dim3(kMkOpenThreads), args, 0, (hipStream_t)stream));
	return BN_OK;
}

extern "C" int bn_merkle_hash_leaf(const void* leaf, int log_leaf_elems, uint8_t* out32) {
	BN_CHECK_ARG(leaf != nullptr && out32 != nullptr, "NULL argument");
	BN_CHECK_ARG(log_leaf_elems >= 0 && log_leaf_elems <= kMkMaxLeafLog, "log_leaf_elems must be in [0, %d] (got %d)", kMkMaxLeafLog,
	             log_leaf_elems);
	mk_hash_leaf((const uint8_t*)leaf, log_leaf_elems, out32);
	return BN_OK;
}

extern "C" int bn_merkle_hash_node(const uint8_t* left32, const uint8_t* right32, uint8_t* out32) {
	BN_CHECK_ARG(left32 != nullptr && right32 != nullptr && out32 != nullptr, "NULL argument");
	mk_hash_node(left32, right32, out32);
	return BN_OK;
}

extern "C" int bn_merkle_verify(const uint8_t* root32, int log_leaves, int log_leaf_elems, uint64_t index, const void* record, int* ok) {
	BN_CHECK_ARG(root32 != nullptr && record != nullptr && ok != nullptr, "NULL argument");
	if (int rc = mk_check_shape(log_leaves, log_leaf_elems)) return rc;
	*ok = mk_verify(root32, log_leaves, log_leaf_elems, index, (const uint8_t*)record) ? 1 : 0;
	return BN_OK;
}

extern "C" int bn_merkle_commit_passes(int log_leaves, int log_leaf_elems, int max_rows, int32_t* out, size_t cap, int* n_passes) {
	BN_CHECK_ARG(out != nullptr && n_passes != nullptr, "NULL argument");
	if (int rc = mk_check_shape(log_leaves, log_leaf_elems)) return rc;
	MkPlan plan;
	BN_CHECK_ARG(mk_plan(log_leaves, log_leaf_elems, max_rows, &plan), "max_rows must be in [0, %d] (got %d)", kMkRowsPerPass, max_rows);
	BN_CHECK_ARG((size_t)plan.n_passes <= cap, "the plan has %d passes, the buffer holds %zu", plan.n_passes, cap);
	for (int p = 0; p < plan.n_passes; p++) {
		out[3 * p] = plan.pass[p].kind;
		out[3 * p + 1] = plan.pass[p].first_row;
		out[3 * p + 2] = plan.pass[p].rows;
	}
	*n_passes = plan.n_passes;
	return BN_OK;
}
