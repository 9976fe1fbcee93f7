// GF(2^128) sumcheck prover on bitsliced columns (Sumcheck<N, d, T>, src/ulvt/sumcheck/sumcheck.cuh).
//
// Semantics (sumcheck.cuh:130-300, fold_batch / compute_sum in core/core.cu): with columns
// f_0..f_{d-1} of cur evaluations and h = cur / 2,
//   points[k] = sum_{x<h} prod_j (f_j(x) + k (f_j(x) + f_j(x+h))),  k = 0..d (tower element k)
//   sum       = points[0] + points[1]   (= sum_{x<cur} prod_j f_j(x); for cur == 1: prod_j f_j(0))
//   fold(r)   : f_j(x) <- f_j(x) + r (f_j(x) + f_j(x+h))   (highest variable first)
//
// Layout: each column is a run of bitsliced 128-word batches (32 elements; word i = bit i of
// the 32 elements, element e in bit e), columns back to back. While cur >= 64 a butterfly pairs
// whole batches x and x + cur/64; below that the single remaining batch pairs bit-lanes.
//
// Arithmetic: one GF(2^128) bitsliced product is spread over a quad of lanes (lane l holds limb
// l = words 32l..32l+31 of each operand and of the result). With A = A_hi X + A_lo the tower's
// top level is done schoolbook (as tower_height_7_mul, tower_7_mul.cu:4-20): lane q computes one
// GF(2^64) product P_q = A_i B_j, (i,j) = (0,0), (1,1), (0,1), (1,0), by Karatsuba over three
// generated GF(2^32) circuits (bsm5_mul); then
//   c_lo = P00 + P11,  c_hi = P01 + P10 + alpha(P11)
// and the quad trades halves through LDS. Operands and partial products travel through a
// 1 KiB LDS slot per quad, so a lane never holds more than ~4 x 32 words of field data.
// The big folds, whose second operand is the wave-uniform challenge, run on lane pairs with
// constant-operand circuits instead (sc_fold_pair).
//
// Round messages are reduced without ever forming 128-word sums: after each product a lane
// folds its 32 result words into one word of parities (bit i = XOR over the elements of bit i),
// which is exactly the limb of the element-sum that the reference's compute_sum produces.
//
// This unit holds the kernels and their launches. Which kernel runs a round, on which grid, is decided
// by the host-only planner (sc_rounds.cpp); the prover's life cycle and rounds are in sc_prover.cpp.
#include <hip/hip_runtime.h>
#include <string.h>

#include <atomic>
#include <chrono>

#include "bitsliced.hpp"
#include "quad_mul.hpp"
#include "sc_prover.hpp"
#include "tower.hpp"

namespace bn {
namespace {

using namespace quad;

// out = k * x for a tower constant k < 16 acting on the 8 GF(2^4) coordinates of a limb; c[a]
// is the GF(2^4) product k * 2^a (host-computed, ScArgs::kcol). Alias-safe.
__device__ __forceinline__ void mul_small(const uint32_t* c, const uint32_t* x, uint32_t* out) {
#pragma unroll
	for (int g = 0; g < 8; g++) {
		uint32_t r[4];
#pragma unroll
		for (int b = 0; b < 4; b++) {
			r[b] = 0;
#pragma unroll
			for (int a = 0; a < 4; a++) r[b] ^= x[4 * g + a] & (0u - ((c[a] >> b) & 1u));
		}
#pragma unroll
		for (int b = 0; b < 4; b++) out[4 * g + b] = r[b];
	}
}

// x <- k x for k = 2 or 3 (m = 0 or ~0: k = 2 + (m & 1)), the same map as mul_small with 8 XORs
// per 4-word group instead of 16 AND-XORs: with X0^2 = X0 + 1, X0 (a0 + a1 X0) = a1 + (a0 + a1) X0 on
// both GF(2^2) halves of each GF(2^4) coordinate, plus m & x
__device__ __forceinline__ void mul_23(uint32_t m, uint32_t* x) {
#pragma unroll
	for (int g = 0; g < 8; g++) {
		const uint32_t b0 = x[4 * g], b1 = x[4 * g + 1], b2 = x[4 * g + 2], b3 = x[4 * g + 3];
		x[4 * g] = b1 ^ (b0 & m);
		x[4 * g + 1] = b0 ^ (b1 & ~m);
		x[4 * g + 2] = b3 ^ (b2 & m);
		x[4 * g + 3] = b2 ^ (b3 & ~m);
	}
}

// bit i = parity of (w[i] & mask): the limb of the sum over the batch's (masked) elements
__device__ __forceinline__ uint32_t parity_word(const uint32_t* w, uint32_t mask) {
	uint32_t r = 0;
#pragma unroll
	for (int i = 0; i < 32; i++) r |= (uint32_t)(__popc(w[i] & mask) & 1) << i;
	return r;
}

struct ScArgs : ScShape {  // the round's shape: d, mode, n_pairs, hb, h, kmax
	uint32_t* cols;
	size_t col_stride;  // words between columns
	int skip1;          // point 1 is not computed (the host derives it from the round claim)
	uint32_t r[4];      // fold challenge
	uint32_t* acc;      // kAccCopies x (kmax + 1) x 4 words, XOR-accumulated (this round's set)
	uint32_t* clr;      // the other accumulator set: cleared here for the next round
	uint32_t* res;      // host-mapped: 4 (kMaxD + 1) point words, then the sequence word
	uint32_t* sink;     // optional device copy of the raw point words + flags (bn_sumcheck_set_message_sink)
	uint32_t seq;       // this launch's sequence number
	int post;           // 1: the last workgroup posts the points (small grids), 0: sc_post does
	uint32_t kcol[kMaxD + 1][4];  // GF(2^4) products k * 2^a (interpolation point k)
	int dbg;            // ScKnobs::dbg (BN_SC_DBG; 0 in the product build)
};

// The development build's BN_SC_DBG bits (sc_rounds.hpp); constant false in the product build, so
// the branches on it compile away.
#ifdef BN_DEV
__device__ __forceinline__ bool dbg(const ScArgs& A, int bit) { return (A.dbg & bit) != 0; }
#else
constexpr bool dbg(const ScArgs&, int) { return false; }
#endif

// lo/hi limbs of column j for pair p (this lane's limb l)
template <int MODE>
__device__ __forceinline__ void load_pair(const ScArgs& A, int j, size_t p, int l, uint32_t* lo, uint32_t* hi, uint32_t& emask) {
	const uint32_t* c = A.cols + (size_t)j * A.col_stride;
	if (dbg(A, 1)) {  // synthetic operands
#pragma unroll
		for (int i = 0; i < 32; i++) {
			lo[i] = (uint32_t)p * 0x9E3779B9u + (uint32_t)(i * 7 + l + j);
			hi[i] = lo[i] * 0x85EBCA6Bu;
		}
		emask = ~0u;
		return;
	}
	if constexpr (MODE == 0) {
		ld32(lo, c + 128 * p + 32 * l);
		ld32(hi, c + 128 * (p + A.hb) + 32 * l);
		emask = ~0u;
	} else if constexpr (MODE == 1) {
		const uint32_t m = (1u << A.h) - 1u;
		uint32_t w[32];
		ld32(w, c + 32 * l);
#pragma unroll
		for (int i = 0; i < 32; i++) {
			lo[i] = w[i] & m;
			hi[i] = (w[i] >> A.h) & m;
		}
		emask = m;
	} else {
		ld32(lo, c + 32 * l);
#pragma unroll
		for (int i = 0; i < 32; i++) {
			lo[i] &= 1u;
			hi[i] = lo[i];  // k = 0 only: f = lo
		}
		emask = 1u;
	}
}

// f_j at point k from its pair: lo <- lo + k (lo + hi) (hi is scratch); kcol[k] as ScArgs::kcol
__device__ __forceinline__ void point_at(const ScArgs& A, const uint32_t (*kcol)[4], int k, uint32_t* lo, uint32_t* hi) {
	if (k == 0) {
	} else if (k == 1) {
#pragma unroll
		for (int i = 0; i < 32; i++) lo[i] = hi[i];
	} else {
#pragma unroll
		for (int i = 0; i < 32; i++) hi[i] ^= lo[i];
		if (dbg(A, 4)) {
		} else if (A.kmax <= 3) {  // d <= 3: every k here is 2 or 3 (launch-uniform branch)
			mul_23(0u - (uint32_t)(k & 1), hi);
		} else {
			mul_small(kcol[k], hi, hi);
		}
#pragma unroll
		for (int i = 0; i < 32; i++) lo[i] ^= hi[i];
	}
}

// Post the round: thread t < 4 (kmax + 1) holds point word v. The words go to host-mapped memory
// (and the sink, with its flag word), then, once every thread's stores are fenced, the sequence
// word the host polls. Every thread of the workgroup calls this.
__device__ __forceinline__ void post_words(const ScArgs& A, int t, uint32_t v) {
	if (t < 4 * (A.kmax + 1)) {
		A.res[t] = v;
		if (A.sink) A.sink[t] = v;
	}
	if (A.sink && t == 0) A.sink[kResSeq] = (uint32_t)A.skip1 | (A.mode == 2 ? 2u : 0u);
	__threadfence_system();
	__syncthreads();
	if (t == 0) __hip_atomic_store(A.res + kResSeq, A.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Reduce the accumulator copies and post the points + sequence word to host-mapped memory.
__device__ __forceinline__ void post_points(const ScArgs& A, int t) {
	uint32_t v = 0;
	if (t < 4 * (A.kmax + 1))
		for (int c = 0; c < kAccCopies; c++)
			v ^= __hip_atomic_load(A.acc + c * kAccStride + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	post_words(A, t, v);
}

// Products run on a group of G lanes: G = 4 (quad_mul, throughput) for launches that fill the
// GPU, G = 16 (hex_mul, about a third of the latency) for the last rounds' small launches, G = 64
// (wide_mul, GF(2^16) circuits on 36 lanes) for the smallest. Lanes l < 4 of a group hold the
// limbs of the operands and results.
template <int G>
struct Grp {
	static constexpr int kGroups = kScThreads / G;
	static constexpr int kSlotWords = G == 4 ? kQuadWords : G == 16 ? kHexWords : kWideWords;
	static constexpr int kSlotsWords = kGroups * kSlotWords;
};
template <int G, bool B_SHARED>
__device__ __forceinline__ void grp_mul(const ScArgs& A, const Slot& S, const uint32_t* B, int l) {
	if (dbg(A, 2)) return;  // no products
	if constexpr (G == 4)
		quad_mul<B_SHARED>(S, B, l);
	else if constexpr (G == 16)
		hex_mul<B_SHARED>(S, B, l);
	else
		wide_mul<B_SHARED>(S, B, l);
}

// The workgroup's point sums in LDS, after the product slots and the fold's challenge rows
// ((kMaxD + 1) x 4 words, then the last-workgroup flag and reduction: lds_bytes). Rounds alternate
// between two accumulator sets; the other set was last read back by the previous round's post
// (ordered before this launch), so workgroup 0 clears it here and no memset is queued per round.
// The caller's barrier follows.
template <int G>
__device__ __forceinline__ uint32_t* messages_init(const ScArgs& A, uint32_t* lds) {
	uint32_t* accL = lds + Grp<G>::kSlotsWords + 128;
	if (threadIdx.x < 4 * (kMaxD + 1)) accL[threadIdx.x] = 0;
	if (blockIdx.x == 0)
		for (int i = threadIdx.x; i < kAccSet; i += kScThreads) A.clr[i] = 0;
	return accL;
}

// One messages item on a group of G lanes (lane l of it, slot S): prod_j f_j at point k of pair p,
// its parities XORed into the workgroup's point sums accL. kcol as ScArgs::kcol.
template <int MODE, int G>
__device__ __forceinline__ void message_item(const ScArgs& A, const uint32_t (*kcol)[4], const Slot& S, uint32_t* accL, size_t p,
                                             int k, int l) {
	uint32_t emask = 0;
	for (int j = 0; j < A.d; j++) {
		// f_j at point k, written into the A (j == 0) or B operand
		if (l < 4) {
			uint32_t lo[32], hi[32];
			load_pair<MODE>(A, j, p, l, lo, hi, emask);
			point_at(A, kcol, k, lo, hi);
			sst(S, (j == 0 ? 0 : 4) + l, lo);
		}
		if (j > 0) grp_mul<G, false>(A, S, nullptr, l);
	}
	wsync();
	if (l < 4) {
		uint32_t w[32];
		sld(w, S, l);
		const uint32_t acc = dbg(A, 8) ? w[0] ^ w[31] : parity_word(w, emask);
		if (acc) atomicXor(accL + 4 * k + l, acc);  // LDS atomic
	}
}

// pair and point of messages item `item`: one (pair, point k) per item, k fastest (point 1 left
// out when skip1)
__device__ __forceinline__ void message_pk(const ScArgs& A, size_t item, size_t& p, int& k) {
	const int npts = A.kmax + 1 - A.skip1;
	p = item / npts;
	const int ki = (int)(item % npts);
	k = (A.skip1 && ki >= 1) ? ki + 1 : ki;
}

// The workgroup's reduction and posting, once its items are in accL.
__device__ __forceinline__ void messages_post(const ScArgs& A, uint32_t* accL) {
	const int t = threadIdx.x;
	__syncthreads();
	const int nw = 4 * (A.kmax + 1);
	if (!A.post) {
		if (t < nw && accL[t]) atomicXor(A.acc + (blockIdx.x % kAccCopies) * kAccStride + t, accL[t]);
		return;  // sc_post follows
	}
	if (gridDim.x == 1) {  // a single workgroup posts its own sums
		post_words(A, t, t < nw ? accL[t] : 0u);
		return;
	}
	// small grids (<= kAccCopies workgroups): workgroup b stores its sums into copy b with plain
	// stores, the last one to finish XORs the gridDim.x copies and posts the points itself
	if (t < nw) A.acc[blockIdx.x * kAccStride + t] = accL[t];
	uint32_t* last = accL + 4 * (kMaxD + 1);  // (a static __shared__ word cost a workgroup per CU)
	__syncthreads();
	if (t == 0)
		// acq_rel: release orders this workgroup's stores before its count, acquire makes every other
		// workgroup's stores visible to the last one
		*last = __hip_atomic_fetch_add(A.acc + kAccCount, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
	__syncthreads();
	if (!*last) return;
	__threadfence();
	uint32_t* red = last + 1;  // 4 (kMaxD + 1) words
	if (t < nw) red[t] = 0;
	__syncthreads();
	// every (copy, word) by one thread, XOR-reduced in LDS
	for (int i = t; i < (int)gridDim.x * nw; i += kScThreads) {
		const int b = i / nw, w = i - b * nw;
		const uint32_t v = __hip_atomic_load(A.acc + b * kAccStride + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (v) atomicXor(red + w, v);
	}
	__syncthreads();
	post_words(A, t, t < nw ? red[t] : 0u);
}

// One item per group: the kmax+1 groups of a pair run side by side, so the pair's columns are
// read from HBM once and hit in cache for the other points.
template <int MODE, int G>
__global__ __launch_bounds__(kScThreads, kScMinWG) void sc_messages(ScArgs A) {
	extern __shared__ uint32_t lds[];
	uint32_t* accL = messages_init<G>(A, lds);
	__syncthreads();
	const int l = threadIdx.x % G, qw = threadIdx.x / G;
	size_t p;
	int k;
	message_pk(A, (size_t)blockIdx.x * Grp<G>::kGroups + qw, p, k);
	if (p < A.n_pairs) message_item<MODE, G>(A, A.kcol, Slot{lds + qw * Grp<G>::kSlotWords}, accL, p, k, l);
	messages_post(A, accL);
}

// Big grids: a one-wave kernel after sc_messages reduces the copies and posts the points (one
// counter shared by thousands of workgroups serialised them: 2x the kernel time).
__global__ __launch_bounds__(64) void sc_post(ScArgs A) { post_points(A, threadIdx.x); }

// One fold item on a group of G lanes (lane l of it, slot S): column j's pair p becomes
// lo + r (lo + hi), R the broadcast-bitsliced challenge. In-batch pairs (MODE 1, p = 0): the folded
// values replace the low half's bit-lanes. lo stays in registers across the product (the 16- and
// 64-lane products leave room for it).
template <int MODE, int G>
__device__ __forceinline__ void fold_item(const ScArgs& A, const Slot& S, const uint32_t* R, int j, size_t p, int l) {
	uint32_t lo[32], hi[32], emask;  // (set by the lanes l < 4 that use them)
	if (l < 4) {
		load_pair<MODE>(A, j, p, l, lo, hi, emask);
#pragma unroll
		for (int i = 0; i < 32; i++) hi[i] ^= lo[i];
		sst(S, l, hi);
	}
	grp_mul<G, true>(A, S, R, l);
	if (l >= 4) return;
	sld(hi, S, l);
#pragma unroll
	for (int i = 0; i < 32; i++) lo[i] = (lo[i] ^ hi[i]) & emask;
	wsync();
	st32(A.cols + (size_t)j * A.col_stride + 128 * p + 32 * l, lo);
}

template <int MODE, int G>
__global__ __launch_bounds__(kScThreads, kScMinWG) void sc_fold(ScArgs A) {
	extern __shared__ uint32_t lds[];
	const int l = threadIdx.x % G, qw = threadIdx.x / G;
	uint32_t* R = lds + Grp<G>::kSlotsWords;  // the challenge, broadcast-bitsliced, shared
	if (threadIdx.x < 128) R[threadIdx.x] = 0u - ((A.r[threadIdx.x / 32] >> (threadIdx.x % 32)) & 1u);
	__syncthreads();
	// one item per group (no grid-stride loop: it costs registers)
	const size_t it = (size_t)blockIdx.x * Grp<G>::kGroups + qw;
	if (it < (size_t)A.d * A.n_pairs)
		fold_item<MODE, G>(A, Slot{lds + qw * Grp<G>::kSlotWords}, R, (int)(it / A.n_pairs), it % A.n_pairs, l);
}

// Big-mode fold with wave-coalesced global traffic (n_pairs % 16 == 0): a wave's 16 quads take
// 16 consecutive pairs of one column, so its lo and hi batches are two contiguous 8 KiB runs.
// Lane t moves 16 B at byte 16 t + 1 KiB i (i < 8) and the LDS slots do the transposition to
// the quads' limb rows (sc_fold<0>, one 128-B line per lane per instruction, took 13% longer:
// c4 d=3 round 0, 434 -> 384 us).
__device__ __forceinline__ uint32_t* coal_addr(uint32_t* wslots, int lane, int i) {
	const int w = 4 * lane + 256 * i;  // word offset in the wave's 16-batch run
	return wslots + (w >> 7) * kQuadWords + kRowWords * ((w >> 5) & 3) + (w & 31);
}

__global__ __launch_bounds__(kScThreads, kScMinWG) void sc_fold_coal(ScArgs A) {
	extern __shared__ uint32_t lds[];
	const int l = threadIdx.x & 3, qw = threadIdx.x >> 2, lane = threadIdx.x & 63;
	const Slot S{lds + qw * kQuadWords};
	uint32_t* wslots = lds + (qw & ~15) * kQuadWords;
	uint32_t* R = lds + kQuadsPerWG * kQuadWords;
	if (threadIdx.x < 128) R[threadIdx.x] = 0u - ((A.r[threadIdx.x / 32] >> (threadIdx.x % 32)) & 1u);
	__syncthreads();
	const size_t it0 = (size_t)blockIdx.x * kQuadsPerWG + (qw & ~15);  // the wave's first item
	if (it0 >= (size_t)A.d * A.n_pairs) return;
	const int j = (int)(it0 / A.n_pairs);
	const size_t p0 = it0 % A.n_pairs;
	uint32_t* lo = A.cols + (size_t)j * A.col_stride + 128 * p0;
	const uint32_t* hi = lo + 128 * A.hb;
#pragma unroll
	for (int i = 0; i < 8; i++) {
		const uint4 a = *(const uint4*)(lo + 4 * lane + 256 * i), b = *(const uint4*)(hi + 4 * lane + 256 * i);
		*(uint4*)coal_addr(wslots, lane, i) = make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w);
	}
	grp_mul<4, true>(A, S, R, l);
	wsync();
#pragma unroll
	for (int i = 0; i < 8; i++) {
		const uint4 a = *(const uint4*)(lo + 4 * lane + 256 * i), q = *(const uint4*)coal_addr(wslots, lane, i);
		*(uint4*)(lo + 4 * lane + 256 * i) = make_uint4(a.x ^ q.x, a.y ^ q.y, a.z ^ q.z, a.w ^ q.w);
	}
}

// Big-mode fold on lane PAIRS (n_pairs % 32 == 0): the product r (lo + hi) has a constant operand,
// the same challenge r for every lane, so its Karatsuba leaves and sums are scalar work. Lane u of
// a pair holds the GF(2^64) half a_u (words 64u..64u+63) of s = lo + hi and forms, with r = r0 +
// r1 X (compact words A.r[0..3]),
//   T = a_u r1            (bsm6_fma_w2: three GF(2^32) circuits whose twiddle side is SGPR bits)
//   the pair swaps T (DPP): lane 0 gets a_1 r1, lane 1 gets a_0 r1
//   lane 0: a_0 r0 + a_1 r1                 = c_lo
//   lane 1: a_1 r0 + a_0 r1 + alpha64(a_1 r1) = c_hi
// (the schoolbook top level of quad_mul with P_ij = a_i r_j). Per product: 6 constant-operand
// GF(2^32) circuits on 2 lanes instead of 12 general ones on 4, and no operand rows in LDS.
// A wave takes 32 consecutive pairs of one column: coalesced 16-B loads as sc_fold_coal, staged
// in LDS rows of 64 words padded to 68 (16 lanes of a ds_read_b128 then hit distinct banks). The
// rows hold s until every lane has read its row, then lo (kept in registers from the loads), so
// the result lo + r s needs no second read of lo from HBM (that re-read was a third of the
// kernel's HBM reads); x stays in registers through both products, opaque to the compiler so the
// two products do not share (and keep live) their data-side sums.
__device__ __forceinline__ uint32_t* pair_addr(uint32_t* slot, int w) { return slot + (w >> 6) * kPairRowWords + (w & 63); }

__global__ __launch_bounds__(kScThreads, kScMinWG) void sc_fold_pair(ScArgs A) {
	extern __shared__ uint32_t lds[];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, u = lane & 1;
	uint32_t* slot = lds + wave * kPairWaveWords;
	const size_t it0 = (size_t)blockIdx.x * kPairItemsPerWG + 32 * wave;  // the wave's first item
	if (it0 >= (size_t)A.d * A.n_pairs) return;
	const int j = (int)(it0 / A.n_pairs);
	const size_t p0 = it0 % A.n_pairs;
	uint32_t* lo = A.cols + (size_t)j * A.col_stride + 128 * p0;
	const uint32_t* hi = lo + 128 * A.hb;
	uint4 la[16];
#pragma unroll
	for (int i = 0; i < 16; i++) {
		const int w = 4 * lane + 256 * i;
		const uint4 b = *(const uint4*)(hi + w);
		la[i] = *(const uint4*)(lo + w);
		*(uint4*)pair_addr(slot, w) = make_uint4(la[i].x ^ b.x, la[i].y ^ b.y, la[i].z ^ b.z, la[i].w ^ b.w);
	}
	wsync();
	uint32_t* row = slot + lane * kPairRowWords;
	uint32_t x[64], t[64];
#pragma unroll
	for (int i = 0; i < 64; i += 4) {
		const uint4 v = *(const uint4*)(row + i);
		x[i] = v.x, x[i + 1] = v.y, x[i + 2] = v.z, x[i + 3] = v.w;
	}
	wsync();  // every row read: the rows take lo
#pragma unroll
	for (int i = 0; i < 16; i++) *(uint4*)pair_addr(slot, 4 * lane + 256 * i) = la[i];
#pragma unroll
	for (int i = 0; i < 64; i++) t[i] = 0;
	if (!dbg(A, 2)) bsm6_fma_w2(x, A.r[2], A.r[3], t);  // a_u r1
	const uint32_t m = 0u - (uint32_t)u;
	uint32_t o[64];
	{
		uint32_t ah[32];
		bs_alpha<5>(t + 32, ah);
#pragma unroll
		for (int i = 0; i < 32; i++) {
			o[i] = (uint32_t)__builtin_amdgcn_mov_dpp((int)t[i], 0xB1, 0xF, 0xF, false) ^ (t[32 + i] & m);
			o[32 + i] = (uint32_t)__builtin_amdgcn_mov_dpp((int)t[32 + i], 0xB1, 0xF, 0xF, false) ^ ((t[i] ^ ah[i]) & m);
		}
	}
	// (x opaque: the compiler would otherwise share the two products' data-side sums)
#pragma unroll
	for (int i = 0; i < 64; i++) asm volatile("" : "+v"(x[i]));
	if (!dbg(A, 2)) bsm6_fma_w2(x, A.r[0], A.r[1], o);  // + a_u r0
	wsync();
#pragma unroll
	for (int i = 0; i < 64; i += 4) {
		const uint4 v = *(const uint4*)(row + i);
		*(uint4*)(row + i) = make_uint4(o[i] ^ v.x, o[i + 1] ^ v.y, o[i + 2] ^ v.z, o[i + 3] ^ v.w);
	}
	wsync();
#pragma unroll
	for (int i = 0; i < 16; i++) {
		const int w = 4 * lane + 256 * i;
		*(uint4*)(lo + w) = *(const uint4*)pair_addr(slot, w);
	}
}

// ---------------------------------------------------------------------------------------
// Round server for the last rounds (at most kServerMaxCur evaluations per column left): ONE
// resident 768-thread workgroup runs every remaining round by itself. It waits for the host's
// challenge in host-mapped control words, folds, computes the next round's messages on 64-lane
// products (wide_mul) and posts them exactly as sc_messages does (points, then the sequence word). A small
// round then costs no kernel launch, no dispatch ramp and no cross-workgroup reduction: with one
// fold and one messages launch per round the last rounds of c4 took ~10 us (fold) + ~18 us
// (messages) of kernel time plus ~12 us of host launches each (round-4 trace).
// A waiting server holds its hardware queue, and work that other streams of the process queue
// behind it on the same queue (HIP maps streams onto a few queues) waits too. So the wait is short
// (kSrvTimeoutTicks of s_memrealtime): a server that gets no challenge in time records the last
// ticket it served (kCtlExit) and ends, and the host relaunches one when it next needs it
// (bn_sumcheck_round_messages). bn_sumcheck_destroy posts kSrvStop.
// ---------------------------------------------------------------------------------------
constexpr uint32_t kSrvStop = 0xFFFFFFFFu;
constexpr int kCtlR = 0, kCtlSkip = 4, kCtlTicket = 5, kCtlExit = 6, kCtlWords = 8;  // host-mapped control words
constexpr uint32_t kSrvRunning = 0xFFFFFFFEu;                   // kCtlExit while a server may be alive
constexpr unsigned long long kSrvTimeoutTicks = 20000ull;        // 200 us at 100 MHz
constexpr int kTraceRounds = 64, kTraceStamps = 4;               // ScKnobs::timing: wake, fold, messages, post

struct SrvArgs {
	uint32_t* cols;
	size_t col_stride;
	int d;
	size_t cur;           // evaluations per column before the first fold
	uint32_t* res;        // host-mapped points + sequence word (as ScArgs::res)
	const uint32_t* ctl;  // host-mapped control words: challenge, skip-p(1) flag, ticket
	uint32_t* ctl_exit;   // ... kCtlExit: the last ticket served by a server that timed out
	uint32_t seq;         // sequence number of the first posted round
	uint32_t ticket;      // ticket of the first challenge
	uint32_t kcol[kMaxD + 1][4];
	unsigned long long* trace;  // ScKnobs::timing: kTraceStamps s_memrealtime stamps per round
};

// phase stamp i of the round on `ticket` (development build with BN_SC_TIMING; nothing otherwise)
__device__ __forceinline__ void srv_stamp(const SrvArgs& P, uint32_t ticket, int i) {
#ifdef BN_DEV
	if (P.trace && threadIdx.x == 0) P.trace[kTraceStamps * (size_t)(ticket % kTraceRounds) + i] = __builtin_amdgcn_s_memrealtime();
#endif
}

__global__ __launch_bounds__(kSrvThreads, 1) void sc_server(SrvArgs P) {
	extern __shared__ uint32_t lds[];
	const int l = threadIdx.x % kSrvG, qw = threadIdx.x / kSrvG;
	const Slot S{lds + qw * Grp<kSrvG>::kSlotWords};
	uint32_t* R = lds + kSrvGroups * Grp<kSrvG>::kSlotWords;  // the challenge, broadcast-bitsliced
	uint32_t* accL = R + 128;                    // (kMaxD + 1) x 4 point words
	uint32_t* ctlL = accL + 4 * (kMaxD + 1);     // [0] wake-up reason, [1] skip-p(1) flag, [2..5] challenge
	ScArgs a{};
	a.cols = P.cols;
	a.col_stride = P.col_stride;
	size_t cur = P.cur;
	uint32_t seq = P.seq, ticket = P.ticket;
	for (;;) {
		// ---- the host's challenge for the fold of this round
		if (threadIdx.x == 0) {
			const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
			uint32_t why = 2;  // timed out
			for (;;) {
				const uint32_t t = __hip_atomic_load(P.ctl + kCtlTicket, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
				if (t == ticket) { why = 0; break; }
				if (t == kSrvStop) { why = 1; break; }
				if (__builtin_amdgcn_s_memrealtime() - t0 > kSrvTimeoutTicks) break;
				__builtin_amdgcn_s_sleep(2);
			}
			ctlL[0] = why;
			// the words the ticket publishes, read by the thread whose acquire saw it
			ctlL[1] = __hip_atomic_load(P.ctl + kCtlSkip, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
			for (int i = 0; i < 4; i++)
				ctlL[2 + i] = __hip_atomic_load(P.ctl + kCtlR + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
		}
		__syncthreads();
		srv_stamp(P, ticket, 0);
		if (ctlL[0] != 0) {
			// timed out: tell the host which ticket was served last (it relaunches for the next)
			if (ctlL[0] == 2 && threadIdx.x == 0)
				__hip_atomic_store(P.ctl_exit, ticket - 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
			return;
		}
		if (threadIdx.x < 128) R[threadIdx.x] = 0u - ((ctlL[2 + threadIdx.x / 32] >> (threadIdx.x % 32)) & 1u);
		if (threadIdx.x < 4 * (kMaxD + 1)) accL[threadIdx.x] = 0;
		__syncthreads();
		// ---- fold: cur -> cur / 2, the groups striding over the items
		static_cast<ScShape&>(a) = sc_shape(cur, P.d);
		for (size_t it = qw; it < (size_t)a.d * a.n_pairs; it += kSrvGroups) {
			const int j = (int)(it / a.n_pairs);
			const size_t p = it % a.n_pairs;
			if (a.mode == 0)
				fold_item<0, kSrvG>(a, S, R, j, p, l);
			else
				fold_item<1, kSrvG>(a, S, R, j, p, l);
			wsync();
		}
		cur /= 2;
		__syncthreads();  // every folded column word is written (one CU: the workgroup's fence suffices)
		srv_stamp(P, ticket, 1);
		// ---- the next round's messages
		static_cast<ScShape&>(a) = sc_shape(cur, P.d);
		a.skip1 = a.mode == 2 ? 0 : (int)(ctlL[1] & 1u);
		for (size_t item = qw; item < a.n_pairs * (size_t)(a.kmax + 1 - a.skip1); item += kSrvGroups) {
			size_t p;
			int k;
			message_pk(a, item, p, k);
			if (a.mode == 0)
				message_item<0, kSrvG>(a, P.kcol, S, accL, p, k, l);
			else if (a.mode == 1)
				message_item<1, kSrvG>(a, P.kcol, S, accL, p, k, l);
			else
				message_item<2, kSrvG>(a, P.kcol, S, accL, p, k, l);
			wsync();
		}
		__syncthreads();
		srv_stamp(P, ticket, 2);
		if (threadIdx.x < 4 * (a.kmax + 1)) P.res[threadIdx.x] = accL[threadIdx.x];
		__threadfence_system();
		__syncthreads();
		srv_stamp(P, ticket, 3);
		if (threadIdx.x == 0) __hip_atomic_store(P.res + kResSeq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
		if (cur == 1) return;  // the final evaluation is posted: no fold left
		seq++;
		ticket++;
	}
}

// GF(2^4) products k * 2^a (ScArgs::kcol, SrvArgs::kcol), tabulated once (36 recursive tower
// products per launch were ~1 us of host time on every round's critical path)
struct KCol {
	uint32_t v[kMaxD + 1][4];
	KCol() {
		for (int k = 0; k <= kMaxD; k++)
			for (int a = 0; a < 4; a++) v[k][a] = (uint32_t)tw_mul((uint64_t)k, 1ull << a, 2);
	}
};
const KCol& kcol_table() {
	static const KCol kc;
	return kc;
}

const void* kernel_fn(ScKernel k) {
	switch (k) {
		case ScKernel::Messages0G4: return (const void*)sc_messages<0, 4>;
		case ScKernel::Messages0G16: return (const void*)sc_messages<0, 16>;
		case ScKernel::Messages0G64: return (const void*)sc_messages<0, 64>;
		case ScKernel::Messages1G64: return (const void*)sc_messages<1, 64>;
		case ScKernel::Messages2G64: return (const void*)sc_messages<2, 64>;
		case ScKernel::Fold0G16: return (const void*)sc_fold<0, 16>;
		case ScKernel::Fold1G16: return (const void*)sc_fold<1, 16>;
		case ScKernel::FoldCoal: return (const void*)sc_fold_coal;
		case ScKernel::FoldPair: return (const void*)sc_fold_pair;
	}
	return nullptr;
}

double host_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

volatile uint32_t* ctl(const bn_sumcheck* sc) { return sc->srv.h_ctl; }

}  // namespace

int sc_kernels_init(bn_sumcheck* sc) {
	BN_HIP(hipHostMalloc((void**)&sc->srv.h_ctl, sizeof(uint32_t) * kCtlWords, hipHostMallocMapped | hipHostMallocCoherent));
	memset(sc->srv.h_ctl, 0, sizeof(uint32_t) * kCtlWords);
	BN_HIP(hipFuncSetAttribute((const void*)sc_server, hipFuncAttributeMaxDynamicSharedMemorySize, (int)srv_lds_bytes()));
	for (int k = 0; k < kScKernelCount; k++)
		BN_HIP(hipFuncSetAttribute(kernel_fn((ScKernel)k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sc_max_lds_bytes()));
	return BN_OK;
}

int sc_launch(bn_sumcheck* sc, bool fold, const uint32_t* r) {
	ScArgs A{};
	A.cols = sc->cols;
	A.col_stride = sc->col_words;
	static_cast<ScShape&>(A) = sc_shape(sc->cur, sc->d);
	A.skip1 = (!fold && (sc->have_claim || sc->claim_pending) && A.mode != 2) ? 1 : 0;
	A.res = sc->d_res;
	A.sink = fold ? nullptr : sc->sink;
	if (!fold) A.seq = ++sc->seq;
	A.acc = sc->acc + kAccSet * sc->par;
	A.clr = sc->acc + kAccSet * (1 - sc->par);
	if (fold) memcpy(A.r, r, 16);
	A.dbg = sc->knobs.dbg;
	memcpy(A.kcol, kcol_table().v, sizeof A.kcol);
	const ScLaunch L = sc_plan_launch(A, fold, A.skip1, sc->knobs);
	A.post = L.post;
	void* args[] = {&A};
	BN_HIP(hipLaunchKernel(kernel_fn(L.kernel), dim3((unsigned)L.grid), dim3(L.threads), args, L.lds, sc->stream));
	if (L.post_kernel) BN_HIP(hipLaunchKernel((const void*)sc_post, dim3(1), dim3(64), args, 0, sc->stream));
	return BN_OK;
}

int server_launch(bn_sumcheck* sc, size_t cur, uint32_t seq, uint32_t ticket) {
	SrvArgs P{};
	P.cols = sc->cols;
	P.col_stride = sc->col_words;
	P.d = sc->d;
	P.cur = cur;
	P.res = sc->d_res;
	uint32_t* d_ctl = nullptr;
	BN_HIP(hipHostGetDevicePointer((void**)&d_ctl, sc->srv.h_ctl, 0));
	P.ctl = d_ctl;
	P.ctl_exit = d_ctl + kCtlExit;
	P.seq = seq;
	P.ticket = ticket;
	if (sc->knobs.timing) {
		const size_t bytes = kTraceRounds * kTraceStamps * sizeof(unsigned long long);
		if (!sc->srv.h_trace) {
			BN_HIP(hipHostMalloc((void**)&sc->srv.h_trace, bytes, hipHostMallocMapped | hipHostMallocCoherent));
			memset(sc->srv.h_trace, 0, bytes);
		}
		BN_HIP(hipHostGetDevicePointer((void**)&P.trace, sc->srv.h_trace, 0));
	}
	ctl(sc)[kCtlExit] = kSrvRunning;
	memcpy(P.kcol, kcol_table().v, sizeof P.kcol);
	void* args[] = {&P};
	BN_HIP(hipLaunchKernel((const void*)sc_server, dim3(1), dim3(kSrvThreads), args, srv_lds_bytes(), sc->stream));
	sc->srv.running = true;
	return BN_OK;
}

void server_post(bn_sumcheck* sc, const uint32_t* r, bool skip1) {
	volatile uint32_t* c = ctl(sc);
	for (int i = 0; i < 4; i++) c[kCtlR + i] = r[i];
	c[kCtlSkip] = skip1 ? 1u : 0u;
	std::atomic_thread_fence(std::memory_order_release);
	c[kCtlTicket] = ++sc->srv.ticket;
	sc->seq++;  // the server posts this round's messages with the next sequence number
	if (sc->knobs.timing) sc->srv.t_post = host_us();
}

void server_stop(bn_sumcheck* sc) {
	if (!sc->srv.running || !sc->srv.h_ctl) return;
	std::atomic_thread_fence(std::memory_order_release);
	ctl(sc)[kCtlTicket] = kSrvStop;
}

bool server_exited_at(const bn_sumcheck* sc, uint32_t ticket) { return ctl(sc)[kCtlExit] == ticket; }

// Wait for the round's posted sequence number (the stream is queried between polls, so a failed
// kernel is reported rather than waited for); relaunches a round server that timed out before
// taking this round's challenge.
int wait_posted(bn_sumcheck* sc) {
	const volatile uint32_t* posted = sc->h_res + kResSeq;
	for (;;) {
		bool seen = false;
		for (int i = 0; i < 4096 && !(seen = *posted == sc->seq); i++) {
		}
		if (seen) {
			if (sc->srv.running && sc->srv.h_trace && sc->srv.ticket > 0) {
				const unsigned long long* t = sc->srv.h_trace + kTraceStamps * (size_t)(sc->srv.ticket % kTraceRounds);
				fprintf(stderr, "server round cur=%zu: post->seen %.1f us | wake->fold %.1f fold->msgs %.1f msgs->post %.1f us\n", sc->cur,
				        host_us() - sc->srv.t_post, (t[1] - t[0]) / 100.0, (t[2] - t[1]) / 100.0, (t[3] - t[2]) / 100.0);
			}
			return BN_OK;
		}
		if (sc->srv.running && server_exited_at(sc, sc->srv.ticket - 1)) {
			// the challenge and the ticket are already posted: the new server folds 2 cur down to cur
			std::atomic_thread_fence(std::memory_order_acquire);
			const int lrc = server_launch(sc, sc->cur * 2, sc->seq, sc->srv.ticket);
			if (lrc != BN_OK) return lrc;
			continue;
		}
		const hipError_t e = hipStreamQuery(sc->stream);
		if (e == hipSuccess) {
			if (*posted == sc->seq) return BN_OK;
			// the server may have timed out between the kCtlExit read above and the query (it then
			// records ticket - 1 and ends, so the stream drains without a post): relaunch it
			std::atomic_thread_fence(std::memory_order_acquire);
			if (sc->srv.running && server_exited_at(sc, sc->srv.ticket - 1)) continue;
			BN_FAIL(BN_ERR_HIP, "round messages were not posted (sequence %u)", sc->seq);
		}
		if (e != hipErrorNotReady) BN_FAIL(BN_ERR_HIP, "round messages kernel: %s", hipGetErrorString(e));
	}
}

}  // namespace bn
