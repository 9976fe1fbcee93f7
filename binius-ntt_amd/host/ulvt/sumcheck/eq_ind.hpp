// The eq-indicator expansion over the C-ABI, on __uint128_t values (4 little-endian u32 limbs,
// bigints.cu:6-13). No reference counterpart. Header-only.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../utils/common.hpp"

// E[x] = scale * prod_i (bit_{n-1-i}(x) ? r_i : 1 ^ r_i), x = 0 .. 2^n - 1, n = num_challenges, with
// r_i = challenges[i], highest variable first as evaluate_multilinear_composition takes them; compact
// elements, or the words of the bitsliced blocks. Computed on the GPU.
inline std::vector<__uint128_t> eq_ind_expand(const __uint128_t* challenges, const size_t num_challenges,
                                              const __uint128_t scale = 1, bool bitsliced = false, int device = 0) {
	std::vector<__uint128_t> out(num_challenges <= 30 ? (size_t)1 << num_challenges : 1);
	ulvt::bn_check(bn_eq_expand_host(device, (int)num_challenges, (const uint32_t*)challenges, (const uint32_t*)&scale,
	                                 bitsliced ? 1 : 0, (uint32_t*)out.data()));
	return out;
}

// The same into device memory (2^n elements), asynchronous on `stream` (a hipStream_t, may be null).
inline void eq_ind_expand_device(const __uint128_t* challenges, const size_t num_challenges, void* d_out,
                                 const __uint128_t scale = 1, bool bitsliced = false, void* stream = nullptr) {
	ulvt::bn_check(bn_eq_expand_device((int)num_challenges, (const uint32_t*)challenges, (const uint32_t*)&scale, d_out,
	                                   bitsliced ? 1 : 0, stream));
}

// prod_i (a_i b_i ^ (1 ^ a_i)(1 ^ b_i)): the expansion of a at the point b (host arithmetic).
inline __uint128_t eq_ind_eval(const __uint128_t* a, const __uint128_t* b, const size_t num_vars) {
	__uint128_t out = 0;
	ulvt::bn_check(bn_eq_eval((int)num_vars, (const uint32_t*)a, (const uint32_t*)b, (uint32_t*)&out));
	return out;
}
