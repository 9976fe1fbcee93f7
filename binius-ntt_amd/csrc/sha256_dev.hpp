// SHA-256 compression on the device, one message block per lane, fully unrolled. Ch and Maj are one
// v_bitop3_b32 each, the Sigma and sigma functions three rotates or shifts (v_alignbit_b32) into a
// three-input XOR (v_bitop3_b32), the additions pair up as v_add3_u32. The round constants (and, for a
// constant block, the whole schedule) are instruction literals: the constants are merkle_plan.hpp's.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "merkle_plan.hpp"

namespace bn {

__device__ __forceinline__ uint32_t sha_rotr(uint32_t x, int n) { return __builtin_rotateright32(x, n); }
__device__ __forceinline__ uint32_t sha_xor3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); }
__device__ __forceinline__ uint32_t sha_ch(uint32_t e, uint32_t f, uint32_t g) { return __builtin_amdgcn_bitop3_b32(e, f, g, 0xCA); }   // e ? f : g
__device__ __forceinline__ uint32_t sha_maj(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8); }  // two of three

// round t on the state held in rotating slots: a is s[(0 - t) & 7] .. h is s[(7 - t) & 7]; kw = K[t] + W[t]
__device__ __forceinline__ void sha_round(uint32_t (&s)[8], int t, uint32_t kw) {
	const uint32_t a = s[(0 - t) & 7], b = s[(1 - t) & 7], c = s[(2 - t) & 7];
	const uint32_t e = s[(4 - t) & 7], f = s[(5 - t) & 7], g = s[(6 - t) & 7];
	const uint32_t t1 = s[(7 - t) & 7] + sha_xor3(sha_rotr(e, 6), sha_rotr(e, 11), sha_rotr(e, 25)) + sha_ch(e, f, g) + kw;
	s[(3 - t) & 7] += t1;
	s[(7 - t) & 7] = t1 + sha_xor3(sha_rotr(a, 2), sha_rotr(a, 13), sha_rotr(a, 22)) + sha_maj(a, b, c);
}

// state <- compression of the block w (16 big-endian message words; overwritten by the schedule)
__device__ __forceinline__ void sha256_block(uint32_t (&state)[8], uint32_t (&w)[16]) {
	uint32_t s[8];
#pragma unroll
	for (int i = 0; i < 8; i++) s[i] = state[i];
#pragma unroll
	for (int t = 0; t < 64; t++) {
		if (t >= 16) {
			const uint32_t x = w[(t - 15) & 15], y = w[(t - 2) & 15];
			w[t & 15] += sha_xor3(sha_rotr(x, 7), sha_rotr(x, 18), x >> 3) + w[(t - 7) & 15] + sha_xor3(sha_rotr(y, 17), sha_rotr(y, 19), y >> 10);
		}
		sha_round(s, t, kSha256K[t] + w[t & 15]);
	}
#pragma unroll
	for (int i = 0; i < 8; i++) state[i] += s[i];
}

// K[t] + W[t] of the block that is nothing but the padding of a message of kBytes bytes (a multiple
// of 64): 0x80, zeros, the length in bits
template <uint32_t kBytes>
struct ShaPadSchedule {
	uint32_t kw[64];
	constexpr ShaPadSchedule() : kw{} {
		uint32_t w[64] = {};
		w[0] = 0x80000000u;
		w[15] = kBytes * 8;
		for (int t = 16; t < 64; t++) {
			const uint32_t x = w[t - 15], y = w[t - 2];
			const uint32_t s0 = ((x >> 7) | (x << 25)) ^ ((x >> 18) | (x << 14)) ^ (x >> 3);
			const uint32_t s1 = ((y >> 17) | (y << 15)) ^ ((y >> 19) | (y << 13)) ^ (y >> 10);
			w[t] = w[t - 16] + s0 + w[t - 7] + s1;
		}
		for (int t = 0; t < 64; t++) kw[t] = kSha256K[t] + w[t];
	}
};

// state <- compression of that padding block: rounds only, the schedule is 64 constants
template <uint32_t kBytes>
__device__ __forceinline__ void sha256_pad_block(uint32_t (&state)[8]) {
	static_assert(kBytes % 64 == 0 && kBytes < (1u << 29), "a whole number of blocks, the length in one word");
	constexpr ShaPadSchedule<kBytes> sched{};
	uint32_t s[8];
#pragma unroll
	for (int i = 0; i < 8; i++) s[i] = state[i];
#pragma unroll
	for (int t = 0; t < 64; t++) sha_round(s, t, sched.kw[t]);
#pragma unroll
	for (int i = 0; i < 8; i++) state[i] += s[i];
}

__device__ __forceinline__ void sha256_init(uint32_t (&state)[8]) {
#pragma unroll
	for (int i = 0; i < 8; i++) state[i] = kSha256Init[i];
}

}  // namespace bn
