// Inverse additive NTT over GF(2^32) / GF(2^128): evaluations on one coset back to novel-basis
// coefficients. No reference counterpart (the reference transforms in one direction only).
//
// Semantics: with F_c(x) block c of the forward output (antt.hip), the inverse with coset c maps
// y to the x with F_c(x) = y. The forward butterfly u += w v ; v += u is undone by v += u ;
// u += w v with the same twiddle, and the stages run 0 .. log_h-1 instead of log_h-1 .. 0. The
// plan's subspace table and BsPass tables are used as they are; only the kernels differ.
//
//   antt_inv_v0_group   compact tiles, twiddle recomputed per butterfly (every log_h; variant 0)
//   antt_inv_bs_pass    bitsliced LDS tiles over the forward BsPass tables taken in reverse pass
//                       order (log_h >= 12; variants 1, 4 and 5)
//
// The coset is a launch parameter: one inverse reads n elements and writes n elements, so the tile
// index of the bitsliced passes decomposes into (outer bits, batch) only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "antt_bs.hpp"
#include "antt_bs_dev.hpp"
#include "bitsliced.hpp"
#include "field_dev.hpp"

namespace bn {

// ------------------------------------------------------------------------------------
// Compact inverse: the groups of antt_v0_group taken from the lowest stages upward. A workgroup
// owns a tile of 2^(k+c) elements (the k group bits [lo, lo+k) plus the c lowest index bits)
// staged in LDS; inside the tile the stages ascend with the inverted butterfly.
// ------------------------------------------------------------------------------------
constexpr int kInvTileLog = 12;  // 4096 elements; 64 KiB at 16 B/element

struct InvV0Params {
	const uint32_t* src;  // d_in for the first group (lo == 0), d_out afterwards
	uint32_t* dst;        // d_out
	const uint32_t* s;    // subspace table, log_h x width
	int width;
	int log_h;
	int log_rate;
	int lo, k, c;
	int coset;
};

template <int L>
__global__ __launch_bounds__(256) void antt_inv_v0_group(InvV0Params p) {
	extern __shared__ uint32_t lds[];
	const int tile_log = p.k + p.c;
	const int tile = 1 << tile_log;
	const size_t rest = blockIdx.x;
	const int mid_bits = p.lo - p.c;
	const size_t o_mid = rest & (((size_t)1 << mid_bits) - 1);
	const size_t o_hi = rest >> mid_bits;
	auto gidx = [&](int pos) -> size_t {
		const size_t cc = (size_t)pos & (((size_t)1 << p.c) - 1);
		const size_t g = (size_t)pos >> p.c;
		return (o_hi << (p.lo + p.k)) | (g << p.lo) | (o_mid << p.c) | cc;
	};

	uint8_t* tab = (uint8_t*)(lds + (size_t)tile * L);  // GF(2^8) log/exp tables after the tile
	gf8_tables_to_lds(tab);
	for (int pos = threadIdx.x; pos < tile; pos += blockDim.x) {
		const size_t gi = gidx(pos);
#pragma unroll
		for (int l = 0; l < L; l++) lds[pos * L + l] = p.src[gi * L + l];
	}
	__syncthreads();

	for (int stage = p.lo; stage < p.lo + p.k; stage++) {
		const int b = stage - p.lo + p.c;
		const int npairs = tile >> 1;
		const uint32_t* srow = p.s + (size_t)stage * p.width;
		const int nbits = p.log_h + p.log_rate - 1 - stage;
		for (int q = threadIdx.x; q < npairs; q += blockDim.x) {
			const int pu = ((q >> b) << (b + 1)) | (q & ((1 << b) - 1));
			const int pv = pu | (1 << b);
			const size_t blk = gidx(pu) >> (stage + 1);
			const uint64_t ind = ((uint64_t)p.coset << (p.log_h - 1 - stage)) | (uint64_t)blk;
			uint32_t w = 0;
			for (int kk = 0; kk < nbits; kk++)
				if ((ind >> kk) & 1) w ^= srow[kk];
#pragma unroll
			for (int l = 0; l < L; l++) {
				uint32_t u = lds[pu * L + l], v = lds[pv * L + l];
				v ^= u;
				u ^= (uint32_t)dmul_t<5>(w, v, tab);
				lds[pu * L + l] = u;
				lds[pv * L + l] = v;
			}
		}
		__syncthreads();
	}

	for (int pos = threadIdx.x; pos < tile; pos += blockDim.x) {
		const size_t gi = gidx(pos);
#pragma unroll
		for (int l = 0; l < L; l++) p.dst[gi * L + l] = lds[pos * L + l];
	}
}

int launch_inv_v0(bn_antt_plan* plan, const uint32_t* d_in, uint32_t* d_out, int coset, hipStream_t st) {
	const int log_h = plan->log_h;
	const int L = plan->limbs;
	// the forward groups (launch_v0: balanced passes of <= kInvTileLog stages), lowest first
	const int passes = (log_h + kInvTileLog - 1) / kInvTileLog;
	std::vector<std::pair<int, int>> groups;  // (lo, k)
	for (int hi = log_h, i = 0; hi > 0; i++) {
		const int k = (hi + (passes - i) - 1) / (passes - i);
		groups.push_back({hi - k, k});
		hi -= k;
	}
	std::reverse(groups.begin(), groups.end());
	const void* fn = L == 4 ? (const void*)antt_inv_v0_group<4> : (const void*)antt_inv_v0_group<1>;
	for (const auto& g : groups) {
		const int lo = g.first, k = g.second;
		const int c = std::min(lo, kInvTileLog - k);
		InvV0Params p{lo == 0 ? d_in : d_out, d_out, plan->s_dev, plan->width, log_h, plan->log_rate, lo, k, c, coset};
		const size_t blocks = (size_t)1 << (log_h - k - c);
		const size_t lds = ((size_t)1 << (k + c)) * L * sizeof(uint32_t) + kGf8LdsBytes;
		BN_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
		void* args[] = {&p};
		BN_HIP(hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(256), args, lds, st));
	}
	return BN_OK;
}

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
	BsPass p;
};

template <int L, int ROLE, int FMAX>
__global__ __launch_bounds__(64 * L, 2) void antt_inv_bs_pass(InvBsParams P) {
	extern __shared__ uint32_t lds[];
	constexpr int NT = 64 * L;
	constexpr bool IN_COMPACT = ROLE == ROLE_FIRST || ROLE == ROLE_SINGLE;  // bottom pass
	constexpr bool OUT_COMPACT = ROLE == ROLE_LAST || ROLE == ROLE_SINGLE;
	const BsPass& ps = P.p;
	const int tid = threadIdx.x;
	// wave w owns limb w of the tile for every stage (as antt_bs_pass)
	const int l = tid >> 6, lane = tid & 63;
	uint32_t* plane = lds + l * kPlane;
	uint32_t* cu_w = lds + L * kPlane + l * kMaxStages;  // this wave's copy of the uniform twiddle parts
	const size_t n = (size_t)1 << P.log_h;

	auto tile_off = [&](int q) -> size_t {
		size_t off = 0;
#pragma unroll
		for (int m = 0; m < kBlkBits; m++) off |= (size_t)((q >> m) & 1) << ps.bb[m];
		return off;
	};
	// tile -> (outer bits, batch) -> addresses
	const size_t tile = blockIdx.x;
	const size_t outer = tile & (((size_t)1 << ps.n_outer) - 1);
	const size_t batch = tile >> ps.n_outer;
	size_t outer_off = 0;
	for (int m = 0; m < ps.n_outer; m++) outer_off |= ((outer >> m) & 1) << ps.ob[m];
	uint32_t* dst = P.dst + batch * n * L;
	const uint32_t* src = IN_COMPACT ? (P.src + batch * n * L) : dst;

	uint4 gbuf[kLoads];
#pragma unroll
	for (int r = 0; r < kLoads; r++) {
		if (IN_COMPACT) {
			// compact elements: 16-byte loads, 8*L lanes per 32-element block
			const int u = tid + r * NT;
			const int q = u / (8 * L), j = u % (8 * L);
			gbuf[r] = ld_stream(src + (outer_off | tile_off(q)) * L + 4 * j);
		} else {
			// bitsliced: limb l of block q is 128 contiguous bytes, each wave loads its own plane
			const int u = lane + r * 64;
			const int q = u >> 3, j = u & 7;
			gbuf[r] = ld_stream(src + (outer_off | tile_off(q)) * L + 32 * l + 4 * j);
		}
	}

	// workgroup-uniform twiddle part of every stage (outer bits + the coset), one lane per stage
	if (lane < ps.k) {
		uint32_t c = 0;
		for (int m = 0; m < ps.n_outer; m++) c ^= ps.two[lane][m] & (0u - (uint32_t)((outer >> m) & 1));
		for (int b = 0; b < kMaxRateBits; b++) c ^= ps.twc[lane][b] & (0u - (uint32_t)((P.coset >> b) & 1));
		cu_w[lane] = c;
	}

	// ---- tile into LDS
#pragma unroll
	for (int r = 0; r < kLoads; r++) {
		const uint4 g = gbuf[r];
		if (IN_COMPACT) {
			// split by limb into the planes
			const int u = tid + r * NT;
			const int q = u / (8 * L), j = u % (8 * L);
			const uint32_t w[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
			for (int t = 0; t < 4; t++) {
				const int word = 4 * j + t;
				lds[(word % L) * kPlane + q * kLimbStride + word / L] = w[t];
			}
		} else {
			const int u = lane + r * 64;
			const int q = u >> 3, j = u & 7;
			*(uint4*)(plane + q * kLimbStride + 4 * j) = g;
		}
	}

	auto tile_tw = [&](int j, int q) -> uint32_t {
		uint32_t w = 0;
#pragma unroll
		for (int m = 0; m < kBlkBits; m++) w ^= ps.twt[j][m] & (uint32_t)__builtin_amdgcn_sbfe(q, m, 1);
		return w;
	};
	// the lane's two blocks of the in-word stages and of the transposes
	const int qa = lane, qb = qa | (kTileBlocks / 2);
	uint32_t* pa = plane + qa * kLimbStride;
	uint32_t* pb = plane + qb * kLimbStride;
	auto transpose_own = [&]() {
#pragma unroll
		for (int h = 0; h < 2; h++) {
			uint32_t* x = h ? pb : pa;
			uint32_t r[32];
#pragma unroll
			for (int i = 0; i < 32; i += 4) *(uint4*)(r + i) = *(const uint4*)(x + i);
			transpose32(r);
#pragma unroll
			for (int i = 0; i < 32; i += 4) *(uint4*)(x + i) = *(const uint4*)(r + i);
		}
	};

	if (IN_COMPACT) {
		__syncthreads();  // every wave wrote words of every plane
		transpose_own();
		wave_lds_sync();
		// ---- stages 0..4 (index bits inside the word), lane-private. Per stage v ^= u first, then
		// both blocks share one multiply of the updated v-lanes: A's move down onto the u positions,
		// B's stay on the v positions (the packing and twiddle words of antt_bs_pass).
#pragma unroll 1
		for (int s = 0; s < 5; s++) {  // bottom pass starts at stage 0: j == s
			const uint32_t d = vgpr(1u << s);
			const uint32_t um = vgpr(~lane_mask(s));  // u-lanes (bit s clear)
			const uint32_t cb = cu_w[s] ^ tile_tw(s, qb);
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
#pragma unroll
			for (int i = 0; i < 32; i++) W[i] = ps.pat[s][i] ^ (uint32_t)__builtin_amdgcn_sbfe(cb, i, 1);
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
		const uint32_t w = cu_w[j] ^ tile_tw(j, qu);
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
		// (the condition of antt_bs_pass)
		bool uni = FMAX == 32 && m == kBlkBits - 1 && ps.field[j] == 32;
#pragma unroll
		for (int mm = 0; mm < kBlkBits - 1; mm++) uni = uni && ps.twt[j][mm] == 0u;
		if (uni) {
			asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
			__builtin_amdgcn_sched_barrier(0);
			ntt_mul32_w(V, (uint32_t)__builtin_amdgcn_readfirstlane((int)cu_w[j]), Pr);
			__builtin_amdgcn_sched_barrier(0);
		} else {
#pragma unroll
			for (int i = 0; i < 32; i++) W[i] = (uint32_t)__builtin_amdgcn_sbfe(w, i, 1);
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
		transpose_own();  // back to compact words (lane-private)
		__syncthreads();  // compact elements gather one word from every limb plane
		for (int u = tid; u < kTileBlocks * 8 * L; u += NT) {
			const int q = u / (8 * L), j = u % (8 * L);
			uint32_t w[4];
#pragma unroll
			for (int t = 0; t < 4; t++) {
				const int word = 4 * j + t;
				w[t] = lds[(word % L) * kPlane + q * kLimbStride + word / L];
			}
			st_stream(dst + (outer_off | tile_off(q)) * L + 4 * j, make_uint4(w[0], w[1], w[2], w[3]));
		}
	} else {
#pragma unroll 4
		for (int r = 0; r < kLoads; r++) {
			const int u = lane + r * 64;
			const int q = u >> 3, j = u & 7;
			const uint4 g = *(const uint4*)(plane + q * kLimbStride + 4 * j);
			st_stream(dst + (outer_off | tile_off(q)) * L + 32 * l + 4 * j, g);
		}
	}
}

template <int L, int FMAX>
static const void* inv_kernel_for_f(int role) {
	switch (role) {
		case ROLE_FIRST: return (const void*)antt_inv_bs_pass<L, ROLE_FIRST, FMAX>;
		case ROLE_MID: return (const void*)antt_inv_bs_pass<L, ROLE_MID, FMAX>;
		case ROLE_LAST: return (const void*)antt_inv_bs_pass<L, ROLE_LAST, FMAX>;
		default: return (const void*)antt_inv_bs_pass<L, ROLE_SINGLE, FMAX>;
	}
}
static const void* inv_kernel_for(int L, int role, int fmax) {
	if (L == 4) return fmax <= 8 ? inv_kernel_for_f<4, 8>(role) : inv_kernel_for_f<4, 32>(role);
	return fmax <= 8 ? inv_kernel_for_f<1, 8>(role) : inv_kernel_for_f<1, 32>(role);
}

// tile + one word per stage and wave for the workgroup-uniform twiddle parts (as antt_bs_pass)
static size_t inv_lds_bytes(int L) { return ((size_t)L * kPlane + (size_t)L * kMaxStages) * sizeof(uint32_t); }

int launch_inv_bs(bn_antt_plan* plan, const uint32_t* d_in, uint32_t* d_out, int coset, size_t batch, hipStream_t st) {
	size_t n_passes = 0;
	const BsPass* passes = bs_passes(plan, &n_passes);
	const int L = plan->limbs;
	if (!plan->inv_prepared) {
		for (int role = 0; role < 4; role++)
			for (int f : {8, 32})
				BN_HIP(hipFuncSetAttribute(inv_kernel_for(L, role, f), hipFuncAttributeMaxDynamicSharedMemorySize,
				                           (int)inv_lds_bytes(L)));
		plan->inv_prepared = 1;
	}
	// the forward passes run top stages first and the bottom pass last: the inverse takes them in
	// reverse, so the bottom pass is its first (compact in) and forward pass 0 its last (compact out)
	for (size_t i = n_passes; i-- > 0;) {
		InvBsParams prm;
		prm.src = d_in;
		prm.dst = d_out;
		prm.log_h = plan->log_h;
		prm.coset = coset;
		prm.p = passes[i];
		const bool first = i + 1 == n_passes, last = i == 0;
		const int role = first && last ? ROLE_SINGLE : first ? ROLE_FIRST : last ? ROLE_LAST : ROLE_MID;
		const size_t ntiles = batch << passes[i].n_outer;
		void* args[] = {&prm};
		BN_HIP(hipLaunchKernel(inv_kernel_for(L, role, pass_fmax(passes[i])), dim3((unsigned)ntiles), dim3(64 * L), args,
		                       inv_lds_bytes(L), st));
	}
	return BN_OK;
}

}  // namespace bn
