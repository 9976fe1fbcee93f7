// Ring-switching for GF(2) witnesses over the C-ABI, on __uint128_t values (4 little-endian u32 limbs,
// bigints.cu:6-13; bit v of the value is the basis element beta_v). No reference counterpart.
// Header-only. The protocol the pieces belong to is written out in include/binius_ntt_amd.h.
#pragma once

#include <array>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../utils/common.hpp"

typedef std::array<__uint128_t, 128> RsTable;

// s^_v = XOR over w with bit_v(packed[w]) = 1 of eq[w], v = 0 .. 127, for two bitsliced columns of
// 2^log_n elements (the words of their 128-word blocks). Computed on the GPU, staged through a buffer
// that lives for the call.
inline RsTable rs_partial_evals(const __uint128_t* packed, const __uint128_t* eq, const int log_n, int device = 0) {
	RsTable out{};
	ulvt::bn_check(bn_rs_partial_evals_host(device, (const uint32_t*)packed, (const uint32_t*)eq, log_n, (uint32_t*)out.data()));
	return out;
}

// The same from device memory into device memory (128 elements), asynchronous on `stream` (a
// hipStream_t, may be null).
inline void rs_partial_evals_device(const void* d_packed, const void* d_eq, const int log_n, void* d_out, void* stream = nullptr) {
	ulvt::bn_check(bn_rs_partial_evals_device(d_packed, d_eq, log_n, d_out, stream));
}

// out[w] = XOR over u with bit_u(in[w]) = 1 of matrix[u]: n compact elements, or n 128-word bitsliced
// blocks. Computed on the GPU.
inline std::vector<__uint128_t> gf128_linear_map(const __uint128_t* in, const size_t n, const RsTable& matrix, bool bitsliced = false,
                                                 int device = 0) {
	const size_t elems = bitsliced ? 32 * n : n;
	const bool in_range = n >= 1 && n <= ((size_t)1 << (bitsliced ? 27 : 32));  // else the C-ABI rejects the call
	std::vector<__uint128_t> out(in_range ? elems : 1);
	ulvt::bn_check(bn_gf128_linear_map_host(device, (const uint32_t*)in, n, (const uint32_t*)matrix.data(), bitsliced ? 1 : 0,
	                                        (uint32_t*)out.data()));
	return out;
}

// The same between device buffers (d_out may be d_in), asynchronous on `stream`.
inline void gf128_linear_map_device(const void* d_in, void* d_out, const size_t n, const RsTable& matrix, bool bitsliced = false,
                                    void* stream = nullptr) {
	ulvt::bn_check(bn_gf128_linear_map_device(d_in, d_out, n, (const uint32_t*)matrix.data(), bitsliced ? 1 : 0, stream));
}

// The verifier's arithmetic (host only). r2 and r_low are 7 elements; r_high and rho n elements.
inline RsTable rs_batch_table(const __uint128_t* r2) {
	RsTable out{};
	ulvt::bn_check(bn_rs_batch_table((const uint32_t*)r2, (uint32_t*)out.data()));
	return out;
}

inline __uint128_t rs_row_check(const RsTable& shat, const __uint128_t* r_low) {
	__uint128_t out = 0;
	ulvt::bn_check(bn_rs_row_check((const uint32_t*)shat.data(), (const uint32_t*)r_low, (uint32_t*)&out));
	return out;
}

inline __uint128_t rs_sumcheck_claim(const RsTable& shat, const __uint128_t* r2) {
	__uint128_t out = 0;
	ulvt::bn_check(bn_rs_sumcheck_claim((const uint32_t*)shat.data(), (const uint32_t*)r2, (uint32_t*)&out));
	return out;
}

inline __uint128_t rs_eq_eval(const __uint128_t* r_high, const __uint128_t* rho, const size_t n, const __uint128_t* r2) {
	__uint128_t out = 0;
	ulvt::bn_check(bn_rs_eq_eval((int)n, (const uint32_t*)r_high, (const uint32_t*)rho, (const uint32_t*)r2, (uint32_t*)&out));
	return out;
}
