// Bitsliced, LDS-tiled additive NTT for gfx950 (kernel variant 1).
//
// Data layout
//   * A "block" is 32 consecutive elements. In bitsliced form (the same layout as the
//     reference's BitsliceUtils<128>, src/ulvt/utils/bitslicing.cuh:32-47) block word
//     32*l + i holds bit i of limb l of the 32 elements, element e in bit e.
//   * Between passes the transform lives in HBM as bitsliced blocks in element order (our own
//     scratch layout); the first pass reads the caller's compact AoS input and the last pass
//     writes compact AoS output, so exactly two bit-transposes happen per transform.
//   * A workgroup owns a tile of 128 blocks (2^12 elements, 72 KiB of LDS at GF(2^128), two
//     workgroups per CU so one loads/stores while the other computes): index bits 0..4 inside
//     each word plus 7 "block bits" bb[0..6]; the remaining index bits are fixed per workgroup.
//
// Arithmetic
//   Every twiddle lies in GF(2^32) and multiplies each GF(2^32) limb separately, so a
//   GF(2^128) butterfly is four GF(2^32) bitsliced butterflies sharing one twiddle. Products
//   use the generated Karatsuba circuits (bitsliced_gen.hpp, v_bitop3-fused); the host picks,
//   per stage, the smallest sub-field (GF(2^8)/GF(2^16)/GF(2^32)) that holds every twiddle
//   (multiplication by a sub-field scalar acts on each sub-field coordinate independently).
//   Twiddles are linear in the butterfly-block index (calculate_twiddle, additive_ntt.cuh:
//   59-77): the host tabulates, per stage, the contribution of every tile bit, every fixed
//   (workgroup) index bit and every coset bit, so a twiddle is a handful of masked XORs.
//
// Stage schedule: block-bit stages go through LDS (partners change every stage). In the bottom
// pass the 5 stages on index bits 0..4 pair bit-lanes of one word. A lane owns the same two blocks
// (lane and lane + 64) for all of them and runs them as block stages on a packed pair: one delta
// swap at distance 16 on entry makes word X the elements with index bit 4 clear and Y those with
// it set, stage s is the block-stage butterfly on (X, Y), and a delta swap at distance 2^(s-1)
// on the way back to LDS moves index bit s-1 out of the bit-lane number for the next stage. The
// layout is never restored: the host tabulates the twiddle words for the rotated bit-lane meaning
// (BsPass::pat2), and after stage 0 the transposed pair is written straight to its compact slots.
//
// This file: the two kernel families (antt_bs_pass, antt_bs3_pass), their instances of the list in
// antt_passes.hpp, the launches, and the development build's trace and timing. The pass split, every
// table and the kernel of every launch are planned on the host in antt_passes.cpp.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <type_traits>
#include <vector>

#include "antt_bs.hpp"
#include "antt_bs_dev.hpp"
#include "bitsliced.hpp"
#include "quad_mul.hpp"

namespace bn {

struct BsParams {
	const uint32_t* src;
	uint32_t* dst;
	int log_h, log_rate;
	unsigned long long* trace;  // BN_TRACE=1: per-wave phase timestamps (dev tool)
	int dbg;  // timing experiments only (BN_DEBUG_FLAGS): 1 no loads, 2 no stores, 4 no multiplies
	TileStart ts;        // the pass's tile start and the plan's chunk tables (plan_tile_starts)
	const uint32_t* ut;
	BsPass p;
};

// timing switches and phase traces exist only in the development build (make BN_DEV=1)
#ifdef BN_DEV
#define BS_DBG(P) ((P).dbg)
#define BS_TRACE(P) ((P).trace != nullptr)
#else
#define BS_DBG(P) 0
#define BS_TRACE(P) false
#endif
static_assert(sizeof(BsParams) <= 4096, "BsParams is a kernel argument");

// One pass over every tile: workgroup b transforms tile b.
template <int L, int ROLE, int FMAX>
__device__ __forceinline__ void bs_pass_body(const BsParams& P) {
	extern __shared__ uint32_t lds[];
	constexpr int NT = 64 * L;
	constexpr bool IN_COMPACT = ROLE == ROLE_FIRST || ROLE == ROLE_SINGLE;
	constexpr bool LAST = ROLE == ROLE_LAST || ROLE == ROLE_SINGLE;  // bottom pass, compact out
	// The bottom pass of a transform of two and more passes runs stages 4..0 packed. The
	// single-pass kernel keeps the per-stage pack / multiply / unpack path: with the packed
	// stages in its loop it spills 28 (L = 4) and 23 (L = 1) VGPRs against 9 and 5
	constexpr bool packed = ROLE == ROLE_LAST;
	static_assert(FMAX == 8 || FMAX == 32, "early_u_words is sized for the register use of these two instances");
	static_assert(FMAX == 32 || ROLE == ROLE_FIRST, "only a first pass has every twiddle in GF(2^8) (kNttInstances)");
	constexpr int EARLY = early_u_words(ROLE, FMAX);
	const BsPass& ps = P.p;
	const int tid = threadIdx.x;
	// wave w owns limb w of the tile for every stage: the waves never wait for each other
	// between stages (the four GF(2^32) limb transforms share only their twiddles)
	const int l = tid >> 6, lane = tid & 63;
	uint32_t* plane = lds + l * kPlane;
	uint32_t* cu_w = lds + L * kPlane + l * kMaxStages;  // this wave's copy of the uniform twiddle parts
	const size_t n = (size_t)1 << P.log_h;
	const bool TR = BS_TRACE(P);
	// load, block, in-word, store, (wave-)tiles, pre, mul, post; then the load phase's first two parts:
	// start to last tile load issued, then to tile data complete (the rest of `load`: cu_w ready and
	// the tile in LDS)
	unsigned long long tr[kTraceSlots] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
	auto ts = [&]() -> unsigned long long {
		asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
		return __builtin_amdgcn_s_memtime();
	};
	const unsigned long long t0 = TR ? ts() : 0;

	// tile -> (outer bits, coset, batch) -> addresses
	const TileAddr ta = tile_addr<LAST>(P.ts, P.log_rate);
	const size_t outer_off = ta.outer_off;
	uint32_t* const dst = P.dst + (((ta.batch << P.log_rate) + (size_t)ta.coset) * n) * L;
	const uint32_t* const src = IN_COMPACT ? (P.src + ta.batch * n * L) : dst;
	// the tile's global loads, all in flight at once. Bottom pass: bb[m] = 5 + m (bs_prepare checks
	// it), the tile is one contiguous run of 2^12 elements at outer_off: a workgroup-uniform base and
	// a 32-bit offset per lane
	uint4 gbuf[kLoads];
	auto issue = [&]() {
		if (IN_COMPACT) {
			const uint32_t* const s0 = src + outer_off * L;
#pragma unroll
			for (int r = 0; r < kLoads; r++) {
				const int u = tid + r * NT;
				const uint32_t* g = LAST ? s0 + (uint32_t)(4 * u) : src + compact_off<L>(ps, outer_off, u);
				gbuf[r] = (BS_DBG(P) & 1) ? make_uint4(u, u % (8 * L), u / (8 * L), tid) : ld_stream(g);
			}
		} else {
#pragma unroll
			for (int r = 0; r < kLoads; r++) gbuf[r] = load_plane_bitsliced<L, LAST>(ps, src, outer_off, l, lane, r, BS_DBG(P) & 1);
		}
	};

	// ---- tile-bit stages (index bits >= 5), high to low. Lane = block pair of the wave's limb;
	// V, the twiddle and the first EARLY words of U are live during the multiply, the other words of
	// U are read afterwards.
	// In the bottom pass of a transform of two and more passes the same code runs stages 4..0
	// (index bits inside the word, `inw`) on the
	// packed pair (X, Y) that the lane keeps in the slots of blocks lane and lane + 64 (see
	// pack_pair below): X is U, Y is V, the bit-lane part of the twiddle words comes from
	// BsPass::pat2, and the delta swap for the next stage is applied on the way back to LDS.
	auto block_stage = [&](int j, int pair, bool inw) {
		// the pre / mul / post stamps (tr[5..7]) split the block-stage phase tr[1]: not the in-word stages
		const bool TRB = TR && !inw;
		unsigned long long t_a = TRB ? ts() : 0;
		const int m = inw ? kBlkBits - 1 : ps.stage_m[j];
		const int qu = ((pair >> m) << (m + 1)) | (pair & ((1 << m) - 1));
		const int qv = qu | (1 << m);
		const uint32_t w = cu_w[j] ^ tile_tw(ps, j, qu);
		uint32_t* pu = plane + qu * kLimbStride;
		uint32_t* pv = plane + qv * kLimbStride;
		uint32_t W[32], V[32], Pr[32], U[32];
#pragma unroll
		for (int i = 0; i < 32; i += 4) *(uint4*)(V + i) = *(const uint4*)(pv + i);
		// the first EARLY words of U are requested next to V, ahead of the multiply
#pragma unroll
		for (int i = 0; i < EARLY; i += 4) *(uint4*)(U + i) = *(const uint4*)(pu + i);
		// the stage on the top tile bit with a lane-independent twiddle: scalar twiddle side
		const bool uni = top_stage_uniform<FMAX>(ps, j, m) && !inw && !(BS_DBG(P) & 4);
		if (uni) {
			asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
			__builtin_amdgcn_sched_barrier(0);
			ntt_mul32_w(V, (uint32_t)__builtin_amdgcn_readfirstlane((int)cu_w[j]), Pr);
			__builtin_amdgcn_sched_barrier(0);
		} else {
		if (inw) {
			// the bottom pass starts at stage 0: j is the stage (tw_words(w, ps.pat2[j], W) written out:
			// through the call the GF(2^8) bottom pass at L = 1 takes 129 VGPRs against 128 and loses a
			// wave of occupancy)
#pragma unroll
			for (int i = 0; i < 32; i++) W[i] = ps.pat2[j][i] ^ (uint32_t)__builtin_amdgcn_sbfe(w, i, 1);
		} else {
			tw_words(w, nullptr, W);
		}
		if (TRB) {
			const unsigned long long t = ts();
			tr[5] += t - t_a;
			t_a = t;
		}
		if (BS_DBG(P) & 4) {
#pragma unroll
			for (int i = 0; i < 32; i++) Pr[i] = V[i] ^ W[i];
		} else {
			// V complete before the circuit: with its loads in flight the scheduler hoists the w-side
			// Karatsuba sums to cover their latency, and runs out of registers
			asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
			__builtin_amdgcn_sched_barrier(0);
			mul_tw<FMAX>(ps.field[j], V, W, Pr);  // sub-field circuits reuse W: Pr must not alias it
			__builtin_amdgcn_sched_barrier(0);
		}
		}
		if (TRB) {
			uint32_t acc = 0;
#pragma unroll
			for (int i = 0; i < 32; i++) acc ^= Pr[i];
			asm volatile("" ::"v"(acc));
			const unsigned long long t = ts();
			tr[6] += t - t_a;
			t_a = t;
		}
		if (inw && j > 0) {
			// butterfly, then the delta swap at distance 2^(j-1): X' = index bit j-1 clear, Y' = set,
			// and bit-lane bit j-1 becomes index bit j (shift count and lane mask as VGPR operands: an
			// SGPR operand halves the issue rate)
			const uint32_t d = vgpr(1u << (j - 1));
			const uint32_t um = vgpr(~lane_mask(j - 1));
#pragma unroll
			for (int i = 0; i < 32; i += 4) {
				uint32_t Uw[4], X[4], Y[4];
				*(uint4*)Uw = i < EARLY ? *(const uint4*)(U + i) : *(const uint4*)(pu + i);
#pragma unroll
				for (int t = 0; t < 4; t++) {
					const uint32_t x = Uw[t] ^ Pr[i + t], y = V[i + t] ^ x;
					X[t] = __builtin_amdgcn_bitop3_b32(x, y << d, um, 0xe4);  // (x & um) | (y << d & ~um)
					Y[t] = __builtin_amdgcn_bitop3_b32(x >> d, y, um, 0xe4);  // (x >> d & um) | (y & ~um)
				}
				*(uint4*)(pu + i) = *(const uint4*)X;
				*(uint4*)(pv + i) = *(const uint4*)Y;
			}
		} else {
#pragma unroll
			for (int i = 0; i < 32; i += 4) {
				uint4 u = i < EARLY ? *(const uint4*)(U + i) : *(const uint4*)(pu + i);
				u.x ^= Pr[i];
				u.y ^= Pr[i + 1];
				u.z ^= Pr[i + 2];
				u.w ^= Pr[i + 3];
				*(uint4*)(pu + i) = u;
				*(uint4*)(pv + i) = make_uint4(V[i] ^ u.x, V[i + 1] ^ u.y, V[i + 2] ^ u.z, V[i + 3] ^ u.w);
			}
		}
		if (TRB) tr[7] += ts() - t_a;
	};
	// Entry to the in-word stages (bottom pass). A lane owns blocks A = lane and B = lane + 64,
	// which differ in index bit 11. One delta swap at distance 16 makes X (A's slot) the elements
	// with index bit 4 clear and Y (B's slot) those with it set; bit-lane bit 4 is index bit 11
	// from here on. The stages never return to the canonical layout: at stage s bit-lane bits
	// 0..s-1 are index bits 0..s-1 and bit-lane bits s..3 index bits s+1..4.
	auto pack_pair = [&](uint32_t* pa, uint32_t* pb) {
		const uint32_t d = vgpr(16u), um = vgpr(~lane_mask(4));
#pragma unroll
		for (int i = 0; i < 32; i += 4) {
			uint32_t A[4], Bv[4], X[4], Y[4];
			*(uint4*)A = *(const uint4*)(pa + i);
			*(uint4*)Bv = *(const uint4*)(pb + i);
#pragma unroll
			for (int t = 0; t < 4; t++) {
				X[t] = __builtin_amdgcn_bitop3_b32(A[t], Bv[t] << d, um, 0xe4);
				Y[t] = __builtin_amdgcn_bitop3_b32(A[t] >> d, Bv[t], um, 0xe4);
			}
			*(uint4*)(pa + i) = *(const uint4*)X;
			*(uint4*)(pb + i) = *(const uint4*)Y;
		}
	};

	issue();
	if (TR) {
		const unsigned long long ti = ts();
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		tr[8] += ti - t0;
		tr[9] += ts() - ti;
	}

	// workgroup-uniform twiddle part of every stage (outer + coset bits): four scalar row loads behind
	// the tile's loads in program order, held in SGPRs while the tile moves into LDS and handed to
	// cu_w after it (with the lane word live across the tile's loads and LDS writes instead,
	// antt_bs_pass<4, FIRST, 8> takes 97 VGPRs against 96 and drops from five waves to four)
	__builtin_amdgcn_sched_barrier(0);
	uint32_t cu[kMaxStages];
	uniform_tw_rows(P.ts, P.ut, ta.outer, ta.coset, cu);

	// ---- tile into LDS
	if (IN_COMPACT) {
		// split by limb into the planes, then per-(block, limb) 32x32 transposes of this wave's plane
		// (compact_to_planes written out: through the call the single-pass GF(2^8) kernel at L = 1
		// takes 99 VGPRs against 95 and loses a wave of occupancy)
#pragma unroll
		for (int r = 0; r < kLoads; r++) {
			const uint4 g = gbuf[r];
			const int u = tid + r * NT;
			const int q = u / (8 * L), j = u % (8 * L);
			const uint32_t w[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
			for (int t = 0; t < 4; t++) *plane_word<L>(lds, q, 4 * j + t) = w[t];
		}
		__syncthreads();
		for (int q = lane; q < kTileBlocks; q += 64) transpose_block(plane + q * kLimbStride);
	} else {
		plane_from_regs(plane, lane, gbuf);
	}
	{
		const uint32_t cuv = uniform_tw_to_lanes(cu);  // stage j's word in lane j
		if (lane < kMaxStages) cu_w[lane] = cuv;
	}
	wave_lds_sync();
	unsigned long long t1 = 0;
	if (TR) {
		t1 = ts();
		tr[0] += t1 - t0;
	}

	// the lane's two blocks of the in-word stages and of the transposes
	const int qa = lane, qb = qa | (kTileBlocks / 2);
	uint32_t* pa = plane + qa * kLimbStride;
	uint32_t* pb = plane + qb * kLimbStride;
	// the single-pass kernel stops above the in-word stages: it runs them per stage below
	constexpr int jlow = ROLE == ROLE_SINGLE ? 5 : 0;
	for (int j = ps.k - 1; j >= jlow; j--) {
		const bool inw = packed && j < 5;
		if (packed && j == 4) {
			if (TR) {
				const unsigned long long t = ts();
				tr[1] += t - t1;
				t1 = t;
			}
			pack_pair(pa, pb);
		}
		block_stage(j, lane, inw);
		wave_lds_sync();
	}
	if (TR && !packed) {
		const unsigned long long t = ts();
		tr[1] += t - t1;
		t1 = t;
	}

	if (LAST) {
		// ---- back to compact words (lane-private)
		if (packed) {
			// after stage 0 bit-lane r of X is element 2 (r & 15) of block A (r < 16) or B, and of
			// Y the element after it: pairs go straight to their slots
			uint32_t X[32], Y[32];
#pragma unroll
			for (int i = 0; i < 32; i += 4) *(uint4*)(X + i) = *(const uint4*)(pa + i);
#pragma unroll
			for (int i = 0; i < 32; i += 4) *(uint4*)(Y + i) = *(const uint4*)(pb + i);
			transpose32(X);
			transpose32(Y);
#pragma unroll
			for (int r = 0; r < 32; r += 2)
				*(uint4*)((r & 16 ? pb : pa) + 2 * (r & 15)) = make_uint4(X[r], Y[r], X[r + 1], Y[r + 1]);
		} else {
			// per-stage path: both blocks share one multiply. A's v-lanes move down onto the u
			// positions, B's v-lanes stay on the v positions (a pair's twiddle depends only on
			// index bits above s), and the product is scattered back into A and B
			for (int s = 4; s >= 0; s--) {  // bottom pass starts at stage 0: j == s
				// shift count and lane mask as VGPR operands (an SGPR operand halves the issue rate)
				const uint32_t d = vgpr(1u << s);
				const uint32_t um = vgpr(~lane_mask(s));  // u-lanes (bit s clear)
				const uint32_t cb = cu_w[s] ^ tile_tw(ps, s, qb);
				uint32_t W[32], T[32];
#pragma unroll
				for (int i = 0; i < 32; i += 4) {
					const uint4 a = *(const uint4*)(pa + i), b = *(const uint4*)(pb + i);
					T[i] = __builtin_amdgcn_bitop3_b32(a.x >> d, b.x, um, 0xe4);  // (a>>d & um) | (b & ~um)
					T[i + 1] = __builtin_amdgcn_bitop3_b32(a.y >> d, b.y, um, 0xe4);
					T[i + 2] = __builtin_amdgcn_bitop3_b32(a.z >> d, b.z, um, 0xe4);
					T[i + 3] = __builtin_amdgcn_bitop3_b32(a.w >> d, b.w, um, 0xe4);
				}
				// twiddle word i: pattern (bit-lane bits s+1..4) ^ block part, cb on B's lanes and
				// ca = cb ^ twt[s][6] on A's (um) lanes; the host folds the um & twt[s][6] part into pat
				tw_words(cb, ps.pat[s], W);
				if (BS_DBG(P) & 4) {
#pragma unroll
					for (int i = 0; i < 32; i++) T[i] ^= W[i];
				} else {
					asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // operands complete (see block_stage)
					__builtin_amdgcn_sched_barrier(0);
					mul_tw<FMAX>(ps.field[s], T, W, T);
					__builtin_amdgcn_sched_barrier(0);
				}
#pragma unroll
				for (int i = 0; i < 32; i += 4) {
					uint32_t A[4], Bv[4];
					*(uint4*)A = *(const uint4*)(pa + i);
					*(uint4*)Bv = *(const uint4*)(pb + i);
#pragma unroll
					for (int t = 0; t < 4; t++) {
						// u ^= w*v on the u-lanes, then v ^= u: (x & um) << d == (x << d) & ~um and
						// (x & ~um) >> d == (x >> d) & um for these lane masks
						const uint32_t a = __builtin_amdgcn_bitop3_b32(T[i + t], um, A[t], 0x6a);         // A ^ (T & um)
						const uint32_t b = __builtin_amdgcn_bitop3_b32(T[i + t] >> d, um, Bv[t], 0x6a);  // B ^ ((T >> d) & um)
						A[t] = __builtin_amdgcn_bitop3_b32(a << d, um, a, 0x9a);                          // a ^ ((a << d) & ~um)
						Bv[t] = __builtin_amdgcn_bitop3_b32(b << d, um, b, 0x9a);
					}
					*(uint4*)(pa + i) = *(const uint4*)A;
					*(uint4*)(pb + i) = *(const uint4*)Bv;
				}
			}
			// canonical blocks back to compact words
			transpose_block(pa);
			transpose_block(pb);
		}
		if (TR) {
			const unsigned long long t = ts();
			tr[2] += t - t1;
			t1 = t;
		}
	}

	// ---- store tile
	if (LAST) {
		__syncthreads();  // compact elements gather one word from every limb plane
		// the tile is one contiguous run (see issue()): thread u of iteration it writes 16 bytes at
		// word 4 (u + it NT), and gathers them 8 blocks further on in LDS each time
		uint32_t* const g0 = dst + outer_off * L;
		const int q0 = tid / (8 * L), j0 = tid % (8 * L);
		const uint32_t* sp[4];
#pragma unroll
		for (int t = 0; t < 4; t++) sp[t] = plane_word<L>(lds, q0, 4 * j0 + t);
		constexpr int kStoreIters = kTileBlocks * 8 * L / NT;  // 16
		constexpr int kStepBlocks = NT / (8 * L);              // 8
#pragma unroll
		for (int it = 0; it < kStoreIters; it++) {
			uint32_t w[4];
#pragma unroll
			for (int t = 0; t < 4; t++) w[t] = sp[t][it * kStepBlocks * kLimbStride];
			if (!(BS_DBG(P) & 2)) st_stream(g0 + (uint32_t)(4 * (tid + it * NT)), make_uint4(w[0], w[1], w[2], w[3]));
		}
	} else {
		store_plane_bitsliced<L>(ps, dst, outer_off, l, lane, plane, BS_DBG(P) & 2);
	}
	if (TR) {
		tr[3] += ts() - t1;
		tr[4] += 1;
	}
	if (TR && lane == 0) {
		unsigned long long* o = P.trace + ((size_t)blockIdx.x * (NT / 64) + (tid >> 6)) * kTraceSlots;
		for (int i = 0; i < kTraceSlots; i++) o[i] = tr[i];
	}
}

template <int L, int ROLE, int FMAX>
__global__ __launch_bounds__(64 * L, 2) void antt_bs_pass(BsParams P) {
	bs_pass_body<L, ROLE, FMAX>(P);
}

// ------------------------------------------------------------------------------------
// Lane-split passes (small launches). A pass of T tiles runs 4T waves above; below two tiles per CU
// (one 2^20 transform: 256 tiles, one wave per SIMD) a lone wave issues at half the rate of two
// (DESIGN.md section 5.1). Here each GF(2^32) product of a block pair is split over two waves by the
// tower's top level (v = v0 + v1 X, w = w0 + w1 X over GF(2^16), X^2 = alpha X + 1):
//   wave half 0: (w v)|lo = v0 w0 + v1 w1                 -> words 0..15 of u and v
//   wave half 1: (w v)|hi = v0 w1 + v1 (w0 + alpha w1)    -> words 16..31
// two GF(2^16) products per wave (bsm4, 316 gates: 1264 for the pair against one 1022-gate bsm5)
// and no partial products to exchange. The tile is double-buffered in LDS (a stage reads one copy
// and writes the other), so one work-group barrier per stage orders every access. A work-group is
// 8 waves (4 limbs x 2 halves): two waves per SIMD. Same tiles, tables, HBM layouts and results as
// antt_bs_pass.
// ------------------------------------------------------------------------------------
#define BS3_SB() __builtin_amdgcn_sched_barrier(0)

template <int ROLE>
__global__ __launch_bounds__(kSplitNT, 1) void antt_bs3_pass(BsParams P) {
	static_assert(ROLE == ROLE_FIRST || ROLE == ROLE_MID, "upper passes only: bitsliced out, no in-word stages");
	extern __shared__ uint32_t lds[];
	constexpr int L = 4;
	constexpr bool IN_COMPACT = ROLE == ROLE_FIRST;
	const BsPass& ps = P.p;
	const int tid = threadIdx.x;
	const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
	// BN_TRACE (development build): per-wave cycles of load and its first two parts, block stages,
	// store (tr[0], tr[8], tr[9], tr[1], tr[3]: antt_bs_pass's slots) and of the multiplies inside the
	// block stages (tr[6])
	const bool TR = BS_TRACE(P);
	unsigned long long tr[kTraceSlots] = {0, 0, 0, 0, 1, 0, 0, 0, 0, 0}, tlast = TR ? __builtin_amdgcn_s_memtime() : 0;
	auto mark = [&](int k) {
		if (!TR) return;
		asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
		const unsigned long long t = __builtin_amdgcn_s_memtime();
		tr[k] += t - tlast;
		tlast = t;
	};
	const int l = w & 3, half = w >> 2;  // limb plane, product half
	uint32_t* const cu_w = lds + 8 * kPlane;  // workgroup-uniform twiddle part per stage
	const size_t n = (size_t)1 << P.log_h;
	const TileAddr ta = tile_addr(P.ts, P.log_rate);
	const size_t ooff = ta.outer_off;
	uint32_t* dst = P.dst + (((ta.batch << P.log_rate) + (size_t)ta.coset) * n) * L;
	const uint32_t* src = IN_COMPACT ? (P.src + ta.batch * n * L) : dst;

	// ---- tile into LDS copy 0: 4096 pieces of 16 bytes, 8 per thread, all loads in flight at once
	constexpr int kRounds = (kTileBlocks * 8 * L + kSplitNT - 1) / kSplitNT;
	uint4 g[kRounds];
#pragma unroll
	for (int r = 0; r < kRounds; r++) {
		const int u = tid + r * kSplitNT;
		if (IN_COMPACT) {
			g[r] = ld_stream(src + compact_off<L>(ps, ooff, u));
		} else {
			const int pl = u >> 10, rr = u & 1023, q = rr >> 3, j = rr & 7;  // plane, block, 16-B chunk
			g[r] = ld_stream(src + bitsliced_off<L>(ps, ooff, q, pl, j));
		}
	}
	// workgroup-uniform twiddle part of every stage: scalar loads behind the tile's loads (every wave
	// computes it, wave 0 writes it)
	__builtin_amdgcn_sched_barrier(0);
	const uint32_t cuv = uniform_tw_lanes(P.ts, P.ut, ta.outer, ta.coset);
	if (tid < kMaxStages) cu_w[tid] = cuv;
	mark(8);
	if (TR) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	mark(9);
#pragma unroll
	for (int r = 0; r < kRounds; r++) {
		const int u = tid + r * kSplitNT;
		if (IN_COMPACT) {
			compact_to_planes<L>(lds, u, g[r]);
		} else {
			const int pl = u >> 10, rr = u & 1023, q = rr >> 3, j = rr & 7;
			*(uint4*)(lds + pl * kPlane + q * kLimbStride + 4 * j) = g[r];
		}
	}
	__syncthreads();
	if (IN_COMPACT) {
		// 512 per-(block, limb) 32x32 transposes, one per thread
		transpose_block(lds + (tid >> 7) * kPlane + (tid & 127) * kLimbStride);
		__syncthreads();
	}
	// the stages, instantiated per product half H (its words o = 16 H index register arrays, so they
	// must be compile-time constants); returns the LDS copy holding the tile afterwards
	auto stages = [&](auto hc) -> int {
	constexpr int H = decltype(hc)::value;
	constexpr int o = 16 * H;
	int cur = 0;
	// this wave's half of the product w v: V the 32 operand words, W0 / W1 the twiddle's low / high
	// halves as words (bit i of every bit-lane's 16-bit half in word i). Twiddles of a sub-field
	// (the stage's `field`, wave-uniform) leave W1 zero: half h is then V's half h times W0 alone
	auto half_product = [&](int field, const uint32_t* V, const uint32_t* W0, const uint32_t* W1, uint32_t* p) {
		if (field <= 8) {
			BS3_SB();
			bsm3_mul(V + o, W0, p);
			bsm3_mul(V + o + 8, W0, p + 8);
			BS3_SB();
			return;
		}
		if (field <= 16) {
			BS3_SB();
			bsm4_mul(V + o, W0, p);
			BS3_SB();
			return;
		}
		uint32_t a[16], b[16], z[16];
		if (H == 0) {
#pragma unroll
			for (int i = 0; i < 16; i++) a[i] = W0[i], b[i] = W1[i];
		} else {
			uint32_t al[16];
			quad::bs_alpha<4>(W1, al);
#pragma unroll
			for (int i = 0; i < 16; i++) a[i] = W1[i], b[i] = W0[i] ^ al[i];
		}
		BS3_SB();
		bsm4_mul(V, a, p);
		bsm4_mul(V + 16, b, z);
		BS3_SB();
#pragma unroll
		for (int i = 0; i < 16; i++) p[i] ^= z[i];
	};
	// ---- tile-bit stages: lane = block pair of limb l, as antt_bs_pass
	for (int j = ps.k - 1; j >= 0; j--) {
		const int m = ps.stage_m[j];
		const int qu = ((lane >> m) << (m + 1)) | (lane & ((1 << m) - 1));
		const int qv = qu | (1 << m);
		const uint32_t* su = lds + cur * 4 * kPlane + l * kPlane + qu * kLimbStride;
		const uint32_t* sv = lds + cur * 4 * kPlane + l * kPlane + qv * kLimbStride;
		uint32_t* du = lds + (cur ^ 1) * 4 * kPlane + l * kPlane + qu * kLimbStride;
		uint32_t* dv = lds + (cur ^ 1) * 4 * kPlane + l * kPlane + qv * kLimbStride;
		uint32_t V[32], W0[16], W1[16], pr[16];
#pragma unroll
		for (int i = 0; i < 32; i += 4) *(uint4*)(V + i) = *(const uint4*)(sv + i);
		const uint32_t wt = cu_w[j] ^ tile_tw(ps, j, qu);
#pragma unroll
		for (int i = 0; i < 16; i++) {
			W0[i] = (uint32_t)__builtin_amdgcn_sbfe(wt, i, 1);
			W1[i] = (uint32_t)__builtin_amdgcn_sbfe(wt, 16 + i, 1);
		}
		if (TR) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); tr[6] -= __builtin_amdgcn_s_memtime(); }
		half_product(ps.field[j], V, W0, W1, pr);
		if (TR) { uint32_t acc = 0; for (int q = 0; q < 16; q++) acc ^= pr[q]; asm volatile("" ::"v"(acc)); tr[6] += __builtin_amdgcn_s_memtime(); }
#pragma unroll
		for (int i = 0; i < 16; i += 4) {
			uint4 uu = *(const uint4*)(su + o + i);
			uu.x ^= pr[i], uu.y ^= pr[i + 1], uu.z ^= pr[i + 2], uu.w ^= pr[i + 3];
			*(uint4*)(du + o + i) = uu;
			*(uint4*)(dv + o + i) = make_uint4(V[o + i] ^ uu.x, V[o + i + 1] ^ uu.y, V[o + i + 2] ^ uu.z, V[o + i + 3] ^ uu.w);
		}
		__syncthreads();
		cur ^= 1;
	}
	return cur;
	};
	mark(0);
	tr[0] += tr[8] + tr[9];
	const int cur = half == 0 ? stages(std::integral_constant<int, 0>()) : stages(std::integral_constant<int, 1>());
	mark(1);
	const uint32_t* const fin = lds + cur * 4 * kPlane;
	for (int u = tid; u < kTileBlocks * 8 * L; u += kSplitNT) {
		const int pl = u >> 10, r = u & 1023, q = r >> 3, j = r & 7;
		const uint4 g = *(const uint4*)(fin + pl * kPlane + q * kLimbStride + 4 * j);
		if (!(BS_DBG(P) & 2)) st_stream(dst + bitsliced_off<L>(ps, ooff, q, pl, j), g);
	}
	mark(3);
	if (TR && lane == 0) {
		unsigned long long* o = P.trace + ((size_t)blockIdx.x * (kSplitNT / 64) + w) * kTraceSlots;
		for (int i = 0; i < kTraceSlots; i++) o[i] = tr[i];
	}
}

// ------------------------------------------------------------------------------------
// host: the instances of the two families and their launch (the pass tables and the choice of a
// kernel come from antt_passes.cpp)
// ------------------------------------------------------------------------------------
template <int I>
struct BsAt {
	static const void* fn() {
		constexpr NttInstance k = kNttInstances[I];
		if constexpr (k.family == NttFamily::Bs) return (const void*)antt_bs_pass<k.limbs, k.role, k.fmax>;
		else if constexpr (k.family == NttFamily::Bs3) return (const void*)antt_bs3_pass<k.role>;
		else return nullptr;
	}
};
const void* bs_kernel_fn(int instance) { return instance_table<BsAt>(instance, std::make_index_sequence<kNttInstanceCount>()); }

// BN_TRACE: a zeroed device buffer of kTraceSlots words per wave for one launch
int trace_buffer(size_t waves, hipStream_t st, unsigned long long** out) {
	constexpr size_t kTraceBytes = (size_t)1 << 26;
	static unsigned long long* trbuf = nullptr;
	if (waves * kTraceSlots * sizeof(*trbuf) > kTraceBytes) BN_FAIL(BN_ERR_UNSUPPORTED, "BN_TRACE: %zu waves do not fit the trace buffer", waves);
	if (!trbuf)
		if (int rc = dev_alloc(&trbuf, kTraceBytes)) return rc;
	BN_HIP(hipMemsetAsync(trbuf, 0, waves * kTraceSlots * sizeof(*trbuf), st));
	*out = trbuf;
	return BN_OK;
}
// BN_TRACE: the phase cycles the waves of one launch left in d_trace (kTraceSlots words per wave, the
// slots of tr[] in antt_bs_pass), as averages per wave-tile. The load phase is split into issue (start
// to last tile load issued), data (to tile data complete) and lds (to cu_w ready and the tile in LDS;
// antt_rr_pass: the tile in registers); antt_rr_pass stamps only its load phase
int print_trace(int i, const NttLaunch& nl, int fmax, const unsigned long long* d_trace, size_t waves, hipStream_t st) {
	std::vector<unsigned long long> h(waves * kTraceSlots);
	BN_HIP(hipStreamSynchronize(st));
	BN_HIP(hipMemcpy(h.data(), d_trace, h.size() * sizeof(h[0]), hipMemcpyDeviceToHost));
	double acc[kTraceSlots] = {0};
	for (size_t w = 0; w < waves; w++)
		for (int k = 0; k < kTraceSlots; k++) acc[k] += (double)h[w * kTraceSlots + k];
	const double t = acc[4] > 0 ? acc[4] : 1;  // wave-tiles
	const NttFamily f = kNttInstances[nl.instance].family;
	fprintf(stderr,
	        "trace pass %d (%s, fmax %d, %zu wave-tiles, cycles per wave-tile): load %.0f [issue %.0f data %.0f lds %.0f]  "
	        "block %.0f [pre %.0f mul %.0f post %.0f]  inword+tr %.0f  store %.0f\n",
	        i, f == NttFamily::Rr ? "reg" : f == NttFamily::Bs3 ? "split" : "tile", fmax, (size_t)acc[4], acc[0] / t, acc[8] / t,
	        acc[9] / t, (acc[0] - acc[8] - acc[9]) / t, acc[1] / t, acc[5] / t, acc[6] / t, acc[7] / t, acc[2] / t, acc[3] / t);
	return BN_OK;
}

static int launch_one(bn_antt_plan* plan, int i, const uint32_t* d_in, uint32_t* d_out, size_t batch, hipStream_t st,
                      const BsDevKnobs& kn) {
	const BsPass& pass = plan->passes[i];
	const NttLaunch nl = plan_pass(plan, pass, false, batch, kn);
	if (nl.instance < 0) BN_FAIL(BN_ERR_UNSUPPORTED, "variant %d has no bitsliced passes", plan->variant);
	if (kNttInstances[nl.instance].family == NttFamily::Rr) return rr_launch_pass(plan, i, nl, kn, d_in, d_out, st);
	BsParams prm;
	prm.src = d_in;
	prm.dst = d_out;
	prm.log_h = plan->log_h;
	prm.log_rate = plan->log_rate;
	prm.dbg = kn.dbg;
	prm.ts = plan->starts[i];
	prm.ut = plan->ut_dev;
	prm.p = pass;
	prm.trace = nullptr;
	const size_t waves = nl.grid * (nl.threads / 64);
	if (kn.trace)
		if (int rc = trace_buffer(waves, st, &prm.trace)) return rc;
	int rc = timing_begin(plan, i, st);
	if (rc != BN_OK) return rc;
	void* args[] = {&prm};
	BN_HIP(hipLaunchKernel(bs_kernel_fn(nl.instance), dim3((unsigned)nl.grid), dim3(nl.threads), args, nl.lds, st));
	rc = timing_end(plan, i, st);
	if (rc != BN_OK || !prm.trace) return rc;
	return print_trace(i, nl, pass_fmax(pass), prm.trace, waves, st);
}

// the kernel pass i launches under the plan's variant (variants 1, 4, 5), nullptr otherwise
const void* bs_pass_kernel(bn_antt_plan* plan, int i) {
	if (i < 0 || (size_t)i >= plan->passes.size()) return nullptr;
	// the kernel for ONE transform (bench / profiles): a batched launch of the same pass may pick
	// another (the lane-split and small-bottom kernels depend on the tile count)
	const NttLaunch nl = plan_pass(plan, plan->passes[i], false, 1, bs_dev_knobs());
	return nl.instance < 0 ? nullptr : ntt_kernel_fn(nl.instance);
}

int launch_bs(bn_antt_plan* plan, const uint32_t* d_in, uint32_t* d_out, size_t batch, hipStream_t st) {
	const BsDevKnobs kn = bs_dev_knobs();
	for (size_t i = 0; i < plan->passes.size(); i++) {
		int rc = launch_one(plan, (int)i, d_in, d_out, batch, st, kn);
		if (rc != BN_OK) return rc;
	}
	return BN_OK;
}

// Profiling: each pass launched `reps` times back to back between two hipEvents on `st`
// (steady-state duration per launch, no event between launches). The output buffer holds
// no meaningful values afterwards (passes are re-applied to their own output); the cost of a
// pass does not depend on the values (bitwise arithmetic, no data-dependent control flow).
int bs_time_passes(bn_antt_plan* plan, const uint32_t* d_in, uint32_t* d_out, size_t batch, int reps,
                   hipStream_t st, float* ms, int max_passes, int* n_out) {
	const int n_passes = (int)plan->passes.size();
	BsDevKnobs kn = bs_dev_knobs();
	kn.trace = false;
	const int saved = plan->timing;
	plan->timing = 0;
	hipEvent_t e0 = nullptr, e1 = nullptr;
	int rc = BN_OK;
	if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) rc = BN_ERR_HIP;
	for (int i = 0; rc == BN_OK && i < n_passes; i++) {
		// one untimed launch first: the pass's input is then the steady-state layout
		rc = launch_one(plan, i, d_in, d_out, batch, st, kn);
		if (rc == BN_OK && hipEventRecord(e0, st) != hipSuccess) rc = BN_ERR_HIP;
		for (int r = 0; rc == BN_OK && r < reps; r++) rc = launch_one(plan, i, d_in, d_out, batch, st, kn);
		if (rc == BN_OK && hipEventRecord(e1, st) != hipSuccess) rc = BN_ERR_HIP;
		float t = 0.f;
		if (rc == BN_OK && (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&t, e0, e1) != hipSuccess))
			rc = BN_ERR_HIP;
		if (rc == BN_OK && i < max_passes) ms[i] = t / (float)reps;
	}
	if (e0) (void)hipEventDestroy(e0);
	if (e1) (void)hipEventDestroy(e1);
	plan->timing = saved;
	if (rc != BN_OK) BN_FAIL(rc, "timing the passes failed");
	*n_out = n_passes;
	return BN_OK;
}

}  // namespace bn
