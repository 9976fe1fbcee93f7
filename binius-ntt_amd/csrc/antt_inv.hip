// Inverse additive NTT over GF(2^32) / GF(2^128): evaluations on one coset back to novel-basis
// coefficients. No reference counterpart (the reference transforms in one direction only).
//
// Semantics: with F_c(x) block c of the forward output (antt.hip), the inverse with coset c maps
// y to the x with F_c(x) = y. The forward butterfly u += w v ; v += u is undone by v += u ;
// u += w v with the same twiddle, and the stages run 0 .. log_h-1 instead of log_h-1 .. 0. The
// plan's subspace table and BsPass tables are used as they are; only the kernels differ.
//
//   antt_v0_group<L, true>   compact tiles, twiddle recomputed per butterfly (every log_h; variant
//                            0): the forward's compact kernel, in antt.hip
//   antt_inv_bs_pass         bitsliced LDS tiles over the forward BsPass tables taken in reverse
//                            pass order (log_h >= 12; variants 1, 4 and 5): this file
//
// The coset is a launch parameter: one inverse reads n elements and writes n elements, so the tile
// index of the bitsliced passes decomposes into (outer bits, batch) only.
#include <hip/hip_runtime.h>

#include "antt_bs.hpp"
#include "antt_bs_dev.hpp"
#include "bitsliced.hpp"

namespace bn {

// ------------------------------------------------------------------------------------
// Bitsliced LDS-tile inverse. Same tiles, LDS image (one plane per limb, one wave per limb) and
// HBM layouts as antt_bs_pass; the roles name the position in the inverse's own pass order:
//   ROLE_FIRST   bottom pass: compact in, in-word stages 0..4, block stages 5.., bitsliced out
//   ROLE_MID     upper pass: bitsliced in and out, in place in d_out
//   ROLE_LAST    top pass: bitsliced in, compact out
//   ROLE_SINGLE  log_h == 12: the bottom pass with compact out
// ------------------------------------------------------------------------------------
struct InvBsParams {
	const uint32_t* src;
	uint32_t* dst;
	int log_h;
	int coset;
	TileStart ts;        // the pass's tile start and the plan's chunk tables (plan_tile_starts)
	const uint32_t* ut;
	BsPass p;
};

template <int L, int ROLE, int FMAX>
__global__ __launch_bounds__(64 * L, 2) void antt_inv_bs_pass(InvBsParams P) {
	extern __shared__ uint32_t lds[];
	constexpr int NT = 64 * L;
	constexpr bool IN_COMPACT = ROLE == ROLE_FIRST || ROLE == ROLE_SINGLE;  // bottom pass
	constexpr bool OUT_COMPACT = ROLE == ROLE_LAST || ROLE == ROLE_SINGLE;
	static_assert(FMAX == 32 || (FMAX == 8 && ROLE == ROLE_LAST), "only the top pass has every twiddle in GF(2^8) (kNttInstances)");
	const BsPass& ps = P.p;
	const int tid = threadIdx.x;
	// wave w owns limb w of the tile for every stage (as antt_bs_pass)
	const int l = tid >> 6, lane = tid & 63;
	uint32_t* plane = lds + l * kPlane;
	uint32_t* cu_w = lds + L * kPlane + l * kMaxStages;  // this wave's copy of the uniform twiddle parts
	const size_t n = (size_t)1 << P.log_h;

	// tile -> (outer bits, batch) -> addresses: one coset block in, one out
	const TileAddr ta = tile_addr<IN_COMPACT>(P.ts, 0);
	const size_t outer_off = ta.outer_off;
	uint32_t* dst = P.dst + ta.batch * n * L;
	const uint32_t* src = IN_COMPACT ? (P.src + ta.batch * n * L) : dst;

	// the tile's global loads, all in flight at once
	uint4 gbuf[kLoads];
	if (IN_COMPACT) {
#pragma unroll
		for (int r = 0; r < kLoads; r++) gbuf[r] = ld_stream(src + compact_off<L>(ps, outer_off, tid + r * NT));
	} else {
#pragma unroll
		for (int r = 0; r < kLoads; r++) gbuf[r] = load_plane_bitsliced<L>(ps, src, outer_off, l, lane, r);
	}

	// workgroup-uniform twiddle part of every stage (outer bits + the coset), one lane per stage: scalar
	// loads, behind the tile's loads in program order
	__builtin_amdgcn_sched_barrier(0);
	const uint32_t cuv = uniform_tw_lanes(P.ts, P.ut, ta.outer, P.coset);
	if (lane < kMaxStages) cu_w[lane] = cuv;

	// ---- tile into LDS
	if (IN_COMPACT) {
#pragma unroll
		for (int r = 0; r < kLoads; r++) compact_to_planes<L>(lds, tid + r * NT, gbuf[r]);
	} else {
		plane_from_regs(plane, lane, gbuf);
	}

	// the lane's two blocks of the in-word stages and of the transposes
	const int qa = lane, qb = qa | (kTileBlocks / 2);
	uint32_t* pa = plane + qa * kLimbStride;
	uint32_t* pb = plane + qb * kLimbStride;

	if (IN_COMPACT) {
		__syncthreads();  // every wave wrote words of every plane
		transpose_block(pa);
		transpose_block(pb);
		wave_lds_sync();
		// ---- stages 0..4 (index bits inside the word), lane-private. Per stage v ^= u first, then
		// both blocks share one multiply of the updated v-lanes: A's move down onto the u positions,
		// B's stay on the v positions (the packing and twiddle words of antt_bs_pass).
#pragma unroll 1
		for (int s = 0; s < 5; s++) {  // bottom pass starts at stage 0: j == s
			const uint32_t d = vgpr(1u << s);
			const uint32_t um = vgpr(~lane_mask(s));  // u-lanes (bit s clear)
			const uint32_t cb = cu_w[s] ^ tile_tw(ps, s, qb);
			uint32_t W[32], T[32];
#pragma unroll
			for (int i = 0; i < 32; i += 4) {
				uint32_t A[4], Bv[4];
				*(uint4*)A = *(const uint4*)(pa + i);
				*(uint4*)Bv = *(const uint4*)(pb + i);
#pragma unroll
				for (int t = 0; t < 4; t++) {
					const uint32_t a = __builtin_amdgcn_bitop3_b32(A[t] << d, um, A[t], 0x9a);    // a ^ ((a << d) & ~um)
					const uint32_t b = __builtin_amdgcn_bitop3_b32(Bv[t] << d, um, Bv[t], 0x9a);
					T[i + t] = __builtin_amdgcn_bitop3_b32(a >> d, b, um, 0xe4);  // (a>>d & um) | (b & ~um)
				}
			}
			tw_words(cb, ps.pat[s], W);
			asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // operands complete before the circuit
			__builtin_amdgcn_sched_barrier(0);
			mul_tw<FMAX>(ps.field[s], T, W, T);
			__builtin_amdgcn_sched_barrier(0);
#pragma unroll
			for (int i = 0; i < 32; i += 4) {
				uint32_t A[4], Bv[4];
				*(uint4*)A = *(const uint4*)(pa + i);
				*(uint4*)Bv = *(const uint4*)(pb + i);
#pragma unroll
				for (int t = 0; t < 4; t++) {
					// v ^= u again (cheaper than keeping both blocks live across the circuit), then
					// u ^= w*v on the u-lanes
					const uint32_t a = __builtin_amdgcn_bitop3_b32(A[t] << d, um, A[t], 0x9a);
					const uint32_t b = __builtin_amdgcn_bitop3_b32(Bv[t] << d, um, Bv[t], 0x9a);
					A[t] = __builtin_amdgcn_bitop3_b32(T[i + t], um, a, 0x6a);        // a ^ (T & um)
					Bv[t] = __builtin_amdgcn_bitop3_b32(T[i + t] >> d, um, b, 0x6a);  // b ^ ((T >> d) & um)
				}
				*(uint4*)(pa + i) = *(const uint4*)A;
				*(uint4*)(pb + i) = *(const uint4*)Bv;
			}
		}
	}
	wave_lds_sync();

	// ---- tile-bit stages (index bits >= 5), low to high. Lane = block pair of the wave's limb.
#pragma unroll 1
	for (int j = IN_COMPACT ? 5 : 0; j < ps.k; j++) {
		const int m = ps.stage_m[j];
		const int qu = ((lane >> m) << (m + 1)) | (lane & ((1 << m) - 1));
		const int qv = qu | (1 << m);
		const uint32_t w = cu_w[j] ^ tile_tw(ps, j, qu);
		uint32_t* pu = plane + qu * kLimbStride;
		uint32_t* pv = plane + qv * kLimbStride;
		uint32_t W[32], V[32], Pr[32], U[32];
#pragma unroll
		for (int i = 0; i < 32; i += 4) {
			*(uint4*)(V + i) = *(const uint4*)(pv + i);
			*(uint4*)(U + i) = *(const uint4*)(pu + i);
		}
#pragma unroll
		for (int i = 0; i < 32; i++) V[i] ^= U[i];
		// the stage on the top tile bit with a lane-independent twiddle: scalar twiddle side
		if (top_stage_uniform<FMAX>(ps, j, m)) {
			asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
			__builtin_amdgcn_sched_barrier(0);
			ntt_mul32_w(V, (uint32_t)__builtin_amdgcn_readfirstlane((int)cu_w[j]), Pr);
			__builtin_amdgcn_sched_barrier(0);
		} else {
			tw_words(w, nullptr, W);
			asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
			__builtin_amdgcn_sched_barrier(0);
			mul_tw<FMAX>(ps.field[j], V, W, Pr);  // sub-field circuits reuse W: Pr must not alias it
			__builtin_amdgcn_sched_barrier(0);
		}
#pragma unroll
		for (int i = 0; i < 32; i += 4) {
			// with the small GF(2^8) circuits there are registers to keep U; otherwise read it again
			uint4 u = FMAX <= 8 ? *(const uint4*)(U + i) : *(const uint4*)(pu + i);
			u.x ^= Pr[i];
			u.y ^= Pr[i + 1];
			u.z ^= Pr[i + 2];
			u.w ^= Pr[i + 3];
			*(uint4*)(pu + i) = u;
			*(uint4*)(pv + i) = *(const uint4*)(V + i);
		}
		wave_lds_sync();
	}

	// ---- store tile
	if (OUT_COMPACT) {
		transpose_block(pa);  // back to compact words (lane-private)
		transpose_block(pb);
		__syncthreads();  // compact elements gather one word from every limb plane
		for (int u = tid; u < kTileBlocks * 8 * L; u += NT)
			st_stream(dst + compact_off<L>(ps, outer_off, u), planes_to_compact<L>(lds, u));
	} else {
		store_plane_bitsliced<L>(ps, dst, outer_off, l, lane, plane);
	}
}

template <int I>
struct InvAt {
	static const void* fn() {
		constexpr NttInstance k = kNttInstances[I];
		if constexpr (k.family == NttFamily::InvBs) return (const void*)antt_inv_bs_pass<k.limbs, k.role, k.fmax>;
		return nullptr;
	}
};
const void* inv_kernel_fn(int instance) { return instance_table<InvAt>(instance, std::make_index_sequence<kNttInstanceCount>()); }

int launch_inv_bs(bn_antt_plan* plan, const uint32_t* d_in, uint32_t* d_out, int coset, size_t batch, hipStream_t st) {
	const std::vector<BsPass>& passes = plan->passes;
	const BsDevKnobs kn;  // no development switch touches the inverse
	// the forward passes run top stages first and the bottom pass last: the inverse takes them in
	// reverse, so the bottom pass is its first (compact in) and forward pass 0 its last (compact out)
	for (size_t i = passes.size(); i-- > 0;) {
		const NttLaunch nl = plan_pass(plan, passes[i], true, batch, kn);
		if (nl.instance < 0) BN_FAIL(BN_ERR_UNSUPPORTED, "variant %d has no bitsliced passes", plan->variant);
		InvBsParams prm;
		prm.src = d_in;
		prm.dst = d_out;
		prm.log_h = plan->log_h;
		prm.coset = coset;
		prm.ts = plan->starts[i];
		prm.ut = plan->ut_dev;
		prm.p = passes[i];
		void* args[] = {&prm};
		BN_HIP(hipLaunchKernel(inv_kernel_fn(nl.instance), dim3((unsigned)nl.grid), dim3(nl.threads), args, nl.lds, st));
	}
	return BN_OK;
}

}  // namespace bn
