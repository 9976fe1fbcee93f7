// The bit-reversal permutation of a GF(2^128) column over the C-ABI, on __uint128_t values (4
// little-endian u32 limbs, bigints.cu:6-13). No reference counterpart. Header-only.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "common.hpp"

// out[rev_n(x)] = in[x], x = 0 .. 2^log_n - 1; compact elements, or the words of the bitsliced blocks
// (log_n >= 5). Computed on the GPU, staged through a buffer that lives for the call.
inline std::vector<__uint128_t> bit_reverse(const __uint128_t* in, const int log_n, bool bitsliced = false, int device = 0) {
	std::vector<__uint128_t> out(log_n >= 0 && log_n <= 30 ? (size_t)1 << log_n : 1);
	ulvt::bn_check(bn_bit_reverse_host(device, (const uint32_t*)in, log_n, bitsliced ? 1 : 0, (uint32_t*)out.data()));
	return out;
}

// `batch` columns of 2^log_n elements from device memory to device memory (d_in is not written and
// must not overlap d_out), asynchronous on `stream` (a hipStream_t, may be null).
inline void bit_reverse_device(const void* d_in, void* d_out, const int log_n, size_t batch = 1, bool bitsliced = false,
                               void* stream = nullptr) {
	ulvt::bn_check(bn_bit_reverse_device(d_in, d_out, log_n, batch, bitsliced ? 1 : 0, stream));
}
