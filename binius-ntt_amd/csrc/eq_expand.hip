// The eq-indicator (tensor) expansion of a point r in GF(2^128)^n. No reference counterpart.
//
// Semantics: challenges[i] pairs with index bit n-1-i (highest variable first, the convention of
// bn_multilinear_composition_eval):
//   E[x] = scale * prod_{i<n} ( bit_{n-1-i}(x) ? r_i : 1 ^ r_i )        x = 0 .. 2^n - 1
// One level takes the table A over the k highest variables to k + 1: hi = A[y]*r_k, lo = A[y] ^ hi,
// one product per two results and 2^n - 1 products in all, every one by a launch constant.
//
// Passes (eq_plan.hpp): the n levels are split into passes of at most T = 12 levels, run in place in
// d_out with no scratch. Tile y of a pass with L levels and S levels still to come reads its head
// from d_out[y << (L + S)] (the first pass starts from `scale`) and writes its 2^L results to
// d_out[((y << L) | z) << S]. The head is the tile's own result 0, read before the tile writes
// anything, and no tile reads another's range: stream order between the passes is the only
// synchronisation. The passes before the last write at most 2^(n-T) elements at a stride; the last
// pass writes its 2^T elements contiguously.
//
//   eq_expand_pass  a work-group of 512 threads takes tiles, grid-strided. The tensor product commutes,
//                   so the order of a tile's variables is free: the L - 3 lowest run in LDS, in
//                   place, lowest first (level k: thread t < 2^k reads stage[t], writes the hi half
//                   to stage[t + 2^k] and the lo half back to stage[t]; one product per thread, one
//                   barrier per level), which leaves one element of the stage to each thread. The three
//                   highest run in registers: 7 products and 8 results per thread, result j of
//                   thread t at z = (j << (L - 3)) | t, so consecutive lanes write consecutive
//                   16-byte elements (non-temporal in the last pass). A pass of fewer than three
//                   levels runs them all in LDS and a thread writes one result.
//
// Products: every level of the pass has its nibble table of r in LDS (gf128_rtab.hpp: 8 KiB per
// level, 96 KiB at T = 12, one work-group a CU; two a CU up to 9 levels), built once per resident
// work-group. The tables' unit products r * (1 << j) are r taken through the maps x -> x*X_i of the
// set bits i of j (mul_unit128: integer code, no GF(2^8) tables in this kernel); with dmul128_t, as
// the fold builds them, the twelve tables took three rounds of 512 full products, most of the time
// of a 2^20 expansion. The challenges and the scale travel in the kernel arguments.
//
// Bitsliced output queues the in-place k_bitslice launch (field.hip) behind the last pass.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "eq_plan.hpp"
#include "gf128_rtab.hpp"
#include "stream_io.hpp"

int bitslice_launch(const void* src, void* dst, size_t nblk, int untranspose, hipStream_t st);  // field.hip

namespace bn {

static_assert(kEqRTabBytes == (size_t)kRTabEntries * 16, "eq_plan.hpp's size of a table of r");
static_assert(kEqThreads % 128 == 0, "fold_build_rtab takes 128 threads per table");

struct EqParams {
	uint4* out;
	EqPass pass;
	int first;                   // the heads are `scale` (the first pass: one tile)
	int stream_out;              // non-temporal stores (the last pass)
	unsigned long long n_tiles;
	uint4 scale;
	uint4 r[kEqTileLevels];      // the pass's challenges, highest variable first
};

__device__ __forceinline__ void eq_store(uint4* p, uint4 v, int stream_out) {
	if (stream_out)
		st_stream((uint32_t*)p, v);
	else
		*p = v;
}

__global__ __launch_bounds__(kEqThreads) void eq_expand_pass(EqParams P) {
	extern __shared__ uint4 eq_lds[];
	const int L = P.pass.levels;
	uint4* rtab = eq_lds;                      // [L][32][16]
	uint4* stage = eq_lds + L * kRTabEntries;  // [kEqThreads]
	const int tid = threadIdx.x;

	fold_build_rtab<kEqThreads>(rtab, L, [&](int l, int j) { return mul_unit128(P.r[l], j); });

	const int reg = L >= kEqRegLevels ? kEqRegLevels : 0;  // levels run in registers
	const int lds_levels = L - reg;                         // <= kEqThreadsLog
	for (unsigned long long tile = blockIdx.x; tile < P.n_tiles; tile += gridDim.x) {
		if (tid == 0) stage[0] = P.first ? P.scale : P.out[eq_head_index(P.pass, tile)];
		// ---- LDS level k: bit k of the stage index, the tile's challenge L - 1 - k
#pragma unroll 1
		for (int k = 0; k < lds_levels; k++) {
			__syncthreads();
			if (tid < (1 << k)) {
				const uint4 a = stage[tid];
				const uint4 hi = fold_mul_r(rtab + (L - 1 - k) * kRTabEntries, a);
				stage[tid + (1 << k)] = hi;
				stage[tid] = xor4(a, hi);
			}
		}
		__syncthreads();
		if (tid < (1 << lds_levels)) {
			uint4 v[1 << kEqRegLevels];
			v[0] = stage[tid];
			if (reg) {
				// ---- register levels: bit 2 - i of j pairs with the tile's challenge i
				static_assert(kEqRegLevels == 3, "the register stage is written out for three levels");
				v[4] = fold_mul_r(rtab, v[0]);
				v[0] = xor4(v[0], v[4]);
#pragma unroll
				for (int j = 0; j < 8; j += 4) {
					v[j + 2] = fold_mul_r(rtab + kRTabEntries, v[j]);
					v[j] = xor4(v[j], v[j + 2]);
				}
#pragma unroll
				for (int j = 0; j < 8; j += 2) {
					v[j + 1] = fold_mul_r(rtab + 2 * kRTabEntries, v[j]);
					v[j] = xor4(v[j], v[j + 1]);
				}
#pragma unroll
				for (int j = 0; j < 8; j++)
					eq_store(P.out + eq_out_index(P.pass, tile, ((uint64_t)j << lds_levels) | (unsigned)tid), v[j], P.stream_out);
			} else {
				eq_store(P.out + eq_out_index(P.pass, tile, (unsigned)tid), v[0], P.stream_out);
			}
		}
		__syncthreads();  // the next tile's head goes to stage[0]
	}
}

// Every pass of the plan on `st`, then the bit transpose. Arguments are checked by the caller; the
// current device is the buffer's.
static int eq_launch(int num_vars, const EqPlan& plan, const uint32_t* challenges, const uint32_t* scale, uint4* d_out,
                     int bitsliced, hipStream_t st) {
	int dev = 0, num_cus = 0;
	BN_HIP(hipGetDevice(&dev));
	BN_HIP(hipDeviceGetAttribute(&num_cus, hipDeviceAttributeMultiprocessorCount, dev));
	// up to 104 KiB, above the 64 KiB default: set before every launch (cheap, and correct when the
	// caller switches devices)
	BN_HIP(hipFuncSetAttribute((const void*)eq_expand_pass, hipFuncAttributeMaxDynamicSharedMemorySize,
	                           (int)eq_lds_bytes(kEqTileLevels)));
	const EqPass none{0, 0};  // num_vars == 0: the one result is the head
	const int n_launches = plan.n_passes ? plan.n_passes : 1;
	int at = 0;  // the pass's first challenge
	for (int p = 0; p < n_launches; p++) {
		EqParams prm;
		prm.out = d_out;
		prm.pass = plan.n_passes ? plan.pass[p] : none;
		prm.first = p == 0;
		prm.stream_out = p == n_launches - 1;
		prm.n_tiles = eq_tiles(num_vars, prm.pass);
		prm.scale = scale ? words4(scale) : make_uint4(1, 0, 0, 0);
		for (int i = 0; i < kEqTileLevels; i++)
			prm.r[i] = i < prm.pass.levels ? words4(challenges + 4 * (at + i)) : make_uint4(0, 0, 0, 0);
		at += prm.pass.levels;
		const unsigned grid = (unsigned)eq_grid(prm.n_tiles, prm.pass.levels, num_cus);
		void* args[] = {&prm};
		BN_HIP(hipLaunchKernel((const void*)eq_expand_pass, dim3(grid), dim3(kEqThreads), args, eq_lds_bytes(prm.pass.levels), st));
	}
	if (bitsliced) return bitslice_launch(d_out, d_out, (size_t)1 << (num_vars - 5), 0, st);
	return BN_OK;
}

static int eq_check(int num_vars, const uint32_t* challenges, const void* out, int bitsliced, int max_levels, EqPlan* plan) {
	BN_CHECK_ARG(num_vars >= 0 && num_vars <= kEqMaxVars, "num_vars must be in [0, %d] (got %d)", kEqMaxVars, num_vars);
	BN_CHECK_ARG(out != nullptr, "the output buffer is NULL");
	BN_CHECK_ARG(challenges != nullptr || num_vars == 0, "challenges is NULL");
	BN_CHECK_ARG(!bitsliced || num_vars >= 5, "bitsliced output needs num_vars >= 5 (got %d)", num_vars);
	BN_CHECK_ARG(eq_plan(num_vars, max_levels, plan), "max_levels must be 0 or in [%d, %d] (got %d)", kEqRegLevels,
	             kEqTileLevels, max_levels);
	return BN_OK;
}

}  // namespace bn

using namespace bn;

extern "C" int bn_eq_expand_device_split(int num_vars, const uint32_t* challenges, const uint32_t* scale, void* d_out,
                                         int bitsliced, int max_levels, void* stream) {
	EqPlan plan;
	if (int rc = eq_check(num_vars, challenges, d_out, bitsliced, max_levels, &plan)) return rc;
	return eq_launch(num_vars, plan, challenges, scale, (uint4*)d_out, bitsliced, (hipStream_t)stream);
}

extern "C" int bn_eq_expand_device(int num_vars, const uint32_t* challenges, const uint32_t* scale, void* d_out,
                                   int bitsliced, void* stream) {
	return bn_eq_expand_device_split(num_vars, challenges, scale, d_out, bitsliced, 0, stream);
}

extern "C" int bn_eq_expand_host(int device, int num_vars, const uint32_t* challenges, const uint32_t* scale, int bitsliced,
                                 uint32_t* out) {
	EqPlan plan;
	if (int rc = eq_check(num_vars, challenges, out, bitsliced, 0, &plan)) return rc;
	BN_DEVICE_SCOPE(device);
	const size_t bytes = (size_t)16 << num_vars;
	// staged per call (no input: the challenges travel in the launches): the size depends on num_vars
	DevBuf buf;
	CallStream cs;
	if (int rc = buf.alloc(bytes)) return rc;
	if (int rc = cs.create()) return rc;
	return staged_call(cs.s, nullptr, nullptr, 0, buf.p, out, bytes,
	                   [&](hipStream_t st) { return eq_launch(num_vars, plan, challenges, scale, (uint4*)buf.p, bitsliced, st); });
}

extern "C" int bn_eq_expand_passes(int num_vars, int max_levels, int32_t* levels, size_t cap, int* n_passes) {
	BN_CHECK_ARG(levels != nullptr && n_passes != nullptr, "NULL argument");
	EqPlan plan;
	BN_CHECK_ARG(eq_plan(num_vars, max_levels, &plan), "num_vars must be in [0, %d] and max_levels 0 or in [%d, %d] (got %d, %d)",
	             kEqMaxVars, kEqRegLevels, kEqTileLevels, num_vars, max_levels);
	BN_CHECK_ARG((size_t)plan.n_passes <= cap, "the plan has %d passes, the buffer holds %zu", plan.n_passes, cap);
	for (int p = 0; p < plan.n_passes; p++) levels[p] = plan.pass[p].levels;
	*n_passes = plan.n_passes;
	return BN_OK;
}
