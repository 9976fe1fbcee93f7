// Device helpers shared by the bitsliced kernels of the additive NTT: the forward LDS-tile passes
// (antt_bs.hip), the inverse passes (antt_inv.hip) and the register-tile passes (antt_rr.hip, which
// takes lane_mask and u32x4 from here).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "antt_bs.hpp"
#include "bitsliced.hpp"
#include "bitsliced_ntt_gen.hpp"

namespace bn {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
// streaming (non-temporal) 16-byte global accesses: every byte is touched once per pass
__device__ __forceinline__ uint4 ld_stream(const uint32_t* p) {
	const u32x4 v = __builtin_nontemporal_load((const u32x4*)p);
	return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st_stream(uint32_t* p, uint4 g) {
	u32x4 v;
	v.x = g.x;
	v.y = g.y;
	v.z = g.z;
	v.w = g.w;
	__builtin_nontemporal_store(v, (u32x4*)p);
}

// bit masks of the bit-lanes p with bit j of p set
__host__ __device__ constexpr uint32_t lane_mask(int j) {
	return j == 0 ? 0xAAAAAAAAu : j == 1 ? 0xCCCCCCCCu : j == 2 ? 0xF0F0F0F0u : j == 3 ? 0xFF00FF00u : 0xFFFF0000u;
}

// out = w*x for 32 bitsliced GF(2^32) limbs (alias-safe: out may be x). W holds bit i of each
// lane's twiddle in word i; `field` (uniform per stage) selects the sub-field circuit, FMAX (the
// largest field of the pass) removes the circuits a pass never uses.
template <int FMAX>
__device__ __forceinline__ void mul_tw(int field, const uint32_t* x, const uint32_t* W, uint32_t* out) {
	if (FMAX <= 8 || field <= 8) {
#pragma unroll
		for (int g = 0; g < 4; g++) bsm3_mul(x + 8 * g, W, out + 8 * g);
	} else if (FMAX <= 16 || field <= 16) {
#pragma unroll
		for (int g = 0; g < 2; g++) bsm4_mul(x + 16 * g, W, out + 16 * g);
	} else {
		ntt_mul32(x, W, out);
	}
}

// LDS image of a tile: one plane per limb, block q of limb l at l*kPlane + q*kLimbStride (stride 36
// words: 16 consecutive blocks of one plane hit 16 distinct 4-bank groups, so a wave's
// ds_read_b128 over consecutive blocks is conflict-free).
constexpr int kPlane = kTileBlocks * kLimbStride;
constexpr int kLoads = kTileBlocks * 8 / 64;  // 16-byte global loads per lane per tile

// Stage-to-stage ordering inside one wave: a wave's LDS operations execute in order, so only the
// compiler must not move accesses across this point (the wait also bounds the LDS queue).
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

}  // namespace bn
