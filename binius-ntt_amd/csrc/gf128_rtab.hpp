// Device side of x -> r*x in GF(2^128) for launch constants r, shared by the FRI fold (antt_fold.hip)
// and the eq-indicator expansion (eq_expand.hip). The map is GF(2)-linear, so a work-group
// tabulates it once per constant: r * (e << 4n) for the 32 nibble positions n and the 16 nibble
// values e (8 KiB of LDS per constant, built from the 128 products of r with the unit elements),
// and a product is the XOR of 32 16-byte LDS reads. The 16 entries of a nibble position are 256
// consecutive bytes, one per bank group: lanes with equal nibbles read the same address, lanes with
// different nibbles different banks.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bn {

constexpr int kRTabEntries = 32 * 16;  // uint4 entries of one constant's table

__device__ __forceinline__ uint4 xor4(uint4 a, uint4 b) { return make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w); }
// a GF(2^128) element from its four words (host side: the launch constants travel by value)
inline uint4 words4(const uint32_t* w) { return make_uint4(w[0], w[1], w[2], w[3]); }

// r * x from r's nibble table T[32][16]
__device__ __forceinline__ uint4 fold_mul_r(const uint4* T, uint4 x) {
	const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
	uint4 acc = make_uint4(0, 0, 0, 0);
#pragma unroll
	for (int w = 0; w < 4; w++) {
#pragma unroll
		for (int nib = 0; nib < 8; nib++) acc = xor4(acc, T[(w * 8 + nib) * 16 + ((xs[w] >> (4 * nib)) & 15u)]);
		// at most 16 reads (64 VGPRs) in flight: all 32 at once cost 185 VGPRs, half the waves
		if (w & 1) asm volatile("" : "+v"(acc.x), "+v"(acc.y), "+v"(acc.z), "+v"(acc.w) : : "memory");
	}
	return acc;
}

// x * X_{H-1} in every 2^H-bit block of a word, H <= 5 (tower.hpp's tw_mul_alpha on all the blocks at
// once): (a0 + a1 X)X = a1 + (a0 + a1 X_{H-2}) X
template <int H>
__host__ __device__ __forceinline__ uint32_t mul_x_blocks(uint32_t w) {
	if constexpr (H == 0) {
		return w;
	} else {
		constexpr int half = 1 << (H - 1);
		constexpr uint32_t m = 0xffffffffu / ((1u << half) + 1u);  // the low half of every block
		const uint32_t a0 = w & m, a1 = (w >> half) & m;
		return a1 | ((a0 ^ mul_x_blocks<H - 1>(a1)) << half);
	}
}
// x * X_i in GF(2^128), 0 <= i < 7: the same map on every 2^(i+1)-bit block of the element
template <int I>
__host__ __device__ __forceinline__ uint4 mul_x128(uint4 a) {
	if constexpr (I < 5) {
		return make_uint4(mul_x_blocks<I + 1>(a.x), mul_x_blocks<I + 1>(a.y), mul_x_blocks<I + 1>(a.z), mul_x_blocks<I + 1>(a.w));
	} else if constexpr (I == 5) {  // 64-bit blocks: (lo, hi) -> (hi, lo ^ hi X_4)
		return make_uint4(a.y, a.x ^ mul_x_blocks<5>(a.y), a.w, a.z ^ mul_x_blocks<5>(a.w));
	} else {  // (a0, a1) -> (a1, a0 ^ a1 X_5)
		static_assert(I == 6, "GF(2^128) has X_0 .. X_6");
		return make_uint4(a.z, a.w, a.x ^ a.w, a.y ^ a.z ^ mul_x_blocks<5>(a.w));
	}
}
// r * (1 << j), 0 <= j < 128: bit j of an element is the coefficient of the product of the X_i over
// the set bits i of j, so the unit product is r taken through those maps: seven selects and about
// 150 integer instructions, against the 81 GF(2^8) table products of dmul128_t
__host__ __device__ __forceinline__ uint4 mul_unit128(uint4 r, int j) {
	uint4 t;
	uint32_t m;  // word by word: a select between two uint4 goes through memory
#define BN_MUL_UNIT_STEP(I)                                                      \
	t = mul_x128<I>(r);                                                          \
	m = 0u - (uint32_t)((j >> I) & 1);                                           \
	r = make_uint4(r.x ^ ((r.x ^ t.x) & m), r.y ^ ((r.y ^ t.y) & m), r.z ^ ((r.z ^ t.z) & m), r.w ^ ((r.w ^ t.w) & m));
	BN_MUL_UNIT_STEP(0) BN_MUL_UNIT_STEP(1) BN_MUL_UNIT_STEP(2) BN_MUL_UNIT_STEP(3) BN_MUL_UNIT_STEP(4) BN_MUL_UNIT_STEP(5)
	BN_MUL_UNIT_STEP(6)
#undef BN_MUL_UNIT_STEP
	return r;
}

// The tables of count constants into rtab[count][32][16], by a work-group of kThreads threads (a
// multiple of 128) that all call it. First the unit elements' products, unit(l, j) = r_l * (1 << j)
// (entries 1, 2, 4, 8 of every nibble position; kThreads / 128 constants at a time, 128 threads
// each), then the other entries by linearity. What `unit` reads is synchronised by the caller; the
// tables are synchronised on return.
template <int kThreads, class Unit>
__device__ __forceinline__ void fold_build_rtab(uint4* rtab, int count, Unit unit) {
	const int tid = threadIdx.x;
	for (int l0 = 0; l0 < count; l0 += kThreads / 128) {
		const int l = __builtin_amdgcn_readfirstlane(l0 + (tid >> 7));
		if (l < count) {
			const int j = tid & 127;  // the unit element 1 << j
			rtab[l * kRTabEntries + (j >> 2) * 16 + (1 << (j & 3))] = unit(l, j);
		}
	}
	__syncthreads();
	for (int i = tid; i < count * kRTabEntries; i += kThreads) {
		const int e = i & 15;
		if ((e & (e - 1)) != 0 || e == 0) {  // not a unit entry: those are only read here
			const uint4* units = rtab + (i & ~15);
			uint4 acc = make_uint4(0, 0, 0, 0);
#pragma unroll
			for (int b = 0; b < 4; b++)
				if ((e >> b) & 1) acc = xor4(acc, units[1 << b]);
			rtab[i] = acc;
		}
	}
	__syncthreads();
}

}  // namespace bn
