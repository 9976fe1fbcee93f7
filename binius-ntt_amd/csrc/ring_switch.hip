// Ring-switching for GF(2) witnesses (Diamond-Posen, section 4): the two data-parallel passes over a
// full column that reduce "t(r) = s", t over GF(2), to a sumcheck over the packed column t'. Both are
// GF(2)-linear algebra on 128-bit elements. No reference counterpart.
//
//   rs_partial_evals   s^_v = XOR over w with bit_v(t'[w]) = 1 of E[w], v = 0 .. 127, on two bitsliced
//                      columns (128-word blocks, word b = bit b of the block's 32 elements). Per block
//                      it is the GF(2) matrix product acc[v][u] ^= T[v] & E[u], one v_bitop3 per word
//                      pair; after the last block bit u of s^_v is the parity of acc[v][u].
//                      A work-group takes a contiguous run of blocks, two streams of four waves every
//                      other block of it. Wave k of a stream owns u = 32k .. 32k + 31, lane l owns
//                      v = l and l + 64: 64 accumulator VGPRs. The 32 words of E a wave needs are
//                      wave-uniform (readfirstlane'd offsets: scalar loads, one SGPR operand per
//                      v_bitop3), the two words of T are per lane (two coalesced 256-byte loads a
//                      wave; a stream's four waves read the same lines, three of them from the
//                      vector cache). A lane ends with limb k of s^_l and s^_{l+64};
//                      the streams combine them in LDS (ds atomics) and the work-group adds its 512
//                      words to d_out with vector atomicXor; d_out is zeroed by the call on the same
//                      stream.
//
//   gf128_linear_map   out[w] = XOR over u with bit_u(in[w]) = 1 of matrix[u], any 128 x 128 bit matrix
//                      known at run time. Sixteen byte-indexed tables of 256 entries (64 KiB of LDS,
//                      two work-groups of 512 threads a CU), built once per work-group from the
//                      matrix in the kernel arguments; an element is 16 ds_read_b128 and 16 XORs.
//                      The grid is sized so that a work-group maps at least kMapMinElems elements.
//                      Bitsliced columns run the same kernel between the two bit transposes of
//                      field.hip (k_bitslice), in place in d_out.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.hpp"
#include "gf128_rtab.hpp"
#include "stream_io.hpp"

int bitslice_launch(const void* src, void* dst, size_t nblk, int untranspose, hipStream_t st);  // field.hip

namespace bn {

constexpr int kRsStreams = 2;                    // block streams of four waves each in a work-group
constexpr int kRsThreads = 256 * kRsStreams;
constexpr int kRsMinLog = 5, kRsMaxLog = 30;
constexpr int kRsGroupsPerCu = 3;                // 74 VGPRs: six waves a SIMD
constexpr size_t kRsMinBlocks = 32 * kRsStreams;  // blocks a work-group takes at least (by default)

struct RsParams {
	const uint32_t* __restrict__ packed;
	const uint32_t* __restrict__ eq;
	uint32_t* __restrict__ out;            // 128 x 4 words, zeroed before the launch
	unsigned long long n_blocks, per_group;  // blocks in all and per work-group
};

__global__ __launch_bounds__(kRsThreads) void rs_partial_evals(RsParams P) {
	__shared__ uint32_t red[512];  // the work-group's s^, as d_out lies
	const int lane = threadIdx.x & 63;
	const int wave = __builtin_amdgcn_readfirstlane((threadIdx.x >> 6) & 3);
	const int stream = __builtin_amdgcn_readfirstlane(threadIdx.x >> 8);
	const unsigned long long b0 = (unsigned long long)blockIdx.x * P.per_group;
	const unsigned long long b1 = std::min<unsigned long long>(b0 + P.per_group, P.n_blocks);
	if (threadIdx.x < 512) red[threadIdx.x] = 0;
	uint32_t acc0[32], acc1[32];
#pragma unroll
	for (int j = 0; j < 32; j++) acc0[j] = acc1[j] = 0;
#pragma unroll 2
	for (unsigned long long b = b0 + stream; b < b1; b += kRsStreams) {
		const uint32_t* const t = P.packed + 128 * b;
		const uint32_t* const e = P.eq + 128 * b + 32 * wave;  // uniform: scalar loads
		const uint32_t t0 = __builtin_nontemporal_load(t + lane), t1 = __builtin_nontemporal_load(t + 64 + lane);
#pragma unroll
		for (int j = 0; j < 32; j++) {
			const uint32_t ej = e[j];
			acc0[j] = __builtin_amdgcn_bitop3_b32(t0, ej, acc0[j], 0x6a);  // acc ^ (t & e)
			acc1[j] = __builtin_amdgcn_bitop3_b32(t1, ej, acc1[j], 0x6a);
		}
	}
	uint32_t w0 = 0, w1 = 0;
#pragma unroll
	for (int j = 0; j < 32; j++) {
		w0 |= (uint32_t)(__popc(acc0[j]) & 1) << j;
		w1 |= (uint32_t)(__popc(acc1[j]) & 1) << j;
	}
	// the streams meet in LDS, the work-groups in d_out: 512 atomics a work-group, consecutive lanes
	// consecutive words (one per lane on 2048 work-groups took longer than the blocks at 2^20)
	__syncthreads();
	if (w0) atomicXor(red + 4 * lane + wave, w0);
	if (w1) atomicXor(red + 4 * (lane + 64) + wave, w1);
	__syncthreads();
	if (threadIdx.x < 512 && red[threadIdx.x]) atomicXor(P.out + threadIdx.x, red[threadIdx.x]);
}

constexpr int kMapThreads = 512;
constexpr int kMapBits = 8;  // index bits of a table: one table per byte of the element
constexpr int kMapTables = 128 / kMapBits, kMapEntries = 1 << kMapBits;
constexpr size_t kMapLdsBytes = (size_t)(kMapTables * kMapEntries + 128) * 16;
constexpr size_t kMapMinElems = (size_t)kMapThreads * 16;  // the table build is ~8 elements' work a thread
constexpr int kMapGroupsPerCu = 2;

struct MapParams {
	const uint4* in;
	uint4* out;
	unsigned long long n;
	uint4 matrix[128];
};

__global__ __launch_bounds__(kMapThreads) void gf128_linear_map(MapParams P) {
	extern __shared__ uint4 map_lds[];
	uint4* const tab = map_lds;                            // [kMapTables][kMapEntries]
	uint4* const rows = map_lds + kMapTables * kMapEntries;  // the matrix
	const int tid = threadIdx.x;
	if (tid < 128) rows[tid] = P.matrix[tid];
	__syncthreads();
	for (int i = tid; i < kMapTables * kMapEntries; i += kMapThreads) {
		const uint4* const r = rows + kMapBits * (i >> kMapBits);
		uint4 acc = make_uint4(0, 0, 0, 0);
#pragma unroll
		for (int b = 0; b < kMapBits; b++)
			if ((i >> b) & 1) acc = xor4(acc, r[b]);
		tab[i] = acc;
	}
	__syncthreads();
	const unsigned long long step = (unsigned long long)gridDim.x * kMapThreads;
	for (unsigned long long e = (unsigned long long)blockIdx.x * kMapThreads + tid; e < P.n; e += step) {
		const uint4 x = ld_stream((const uint32_t*)(P.in + e));
		const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
		uint4 acc = make_uint4(0, 0, 0, 0);
#pragma unroll
		for (int w = 0; w < 4; w++)
#pragma unroll
			for (int k = 0; k < 32 / kMapBits; k++)
				acc = xor4(acc, tab[(32 / kMapBits * w + k) * kMapEntries + ((xs[w] >> (kMapBits * k)) & (kMapEntries - 1u))]);
		P.out[e] = acc;
	}
}

static int num_cus(int* n) {
	int dev = 0;
	BN_HIP(hipGetDevice(&dev));
	BN_HIP(hipDeviceGetAttribute(n, hipDeviceAttributeMultiprocessorCount, dev));
	return BN_OK;
}

// Arguments are checked by the caller; the current device is the buffers'.
static int rs_launch(const void* d_packed, const void* d_eq, int log_n, void* d_out, size_t max_blocks_per_group, hipStream_t st) {
	int cus = 0;
	if (int rc = num_cus(&cus)) return rc;
	const size_t n_blocks = (size_t)1 << (log_n - 5);
	size_t per_group = std::max(kRsMinBlocks, (n_blocks + (size_t)cus * kRsGroupsPerCu - 1) / ((size_t)cus * kRsGroupsPerCu));
	if (max_blocks_per_group) per_group = std::min(per_group, max_blocks_per_group);
	const size_t grid = (n_blocks + per_group - 1) / per_group;
	BN_HIP(hipMemsetAsync(d_out, 0, 128 * 16, st));
	RsParams prm;
	prm.packed = (const uint32_t*)d_packed;
	prm.eq = (const uint32_t*)d_eq;
	prm.out = (uint32_t*)d_out;
	prm.n_blocks = n_blocks;
	prm.per_group = per_group;
	void* args[] = {&prm};
	BN_HIP(hipLaunchKernel((const void*)rs_partial_evals, dim3((unsigned)grid), dim3(kRsThreads), args, 0, st));
	return BN_OK;
}

static int rs_check(const void* packed, const void* eq, int log_n, const void* out) {
	BN_CHECK_ARG(packed != nullptr && eq != nullptr && out != nullptr, "NULL buffer");
	BN_CHECK_ARG(log_n >= kRsMinLog && log_n <= kRsMaxLog, "log_n must be in [%d, %d] (got %d)", kRsMinLog, kRsMaxLog, log_n);
	return BN_OK;
}

static int map_launch(const void* d_in, void* d_out, size_t n, const uint32_t* matrix, int bitsliced, hipStream_t st) {
	int cus = 0;
	if (int rc = num_cus(&cus)) return rc;
	const size_t n_elems = bitsliced ? n * 32 : n;
	const void* src = d_in;
	if (bitsliced) {
		if (int rc = bitslice_launch(d_in, d_out, n, 1, st)) return rc;
		src = d_out;
	}
	BN_HIP(hipFuncSetAttribute((const void*)gf128_linear_map, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMapLdsBytes));
	MapParams prm;
	prm.in = (const uint4*)src;
	prm.out = (uint4*)d_out;
	prm.n = n_elems;
	for (int u = 0; u < 128; u++) prm.matrix[u] = words4(matrix + 4 * u);
	const size_t grid = std::min((n_elems + kMapMinElems - 1) / kMapMinElems, (size_t)cus * kMapGroupsPerCu);
	void* args[] = {&prm};
	BN_HIP(hipLaunchKernel((const void*)gf128_linear_map, dim3((unsigned)grid), dim3(kMapThreads), args, kMapLdsBytes, st));
	if (bitsliced) return bitslice_launch(d_out, d_out, n, 0, st);
	return BN_OK;
}

static int map_check(const void* in, const void* out, size_t n, const uint32_t* matrix, int bitsliced) {
	BN_CHECK_ARG(in != nullptr && out != nullptr && matrix != nullptr, "NULL argument");
	BN_CHECK_ARG(n >= 1 && n <= (bitsliced ? (size_t)1 << 27 : (size_t)1 << 32), "n must be in [1, 2^%d] (got %zu)", bitsliced ? 27 : 32,
	             n);
	return BN_OK;
}

}  // namespace bn

using namespace bn;

extern "C" int bn_rs_partial_evals_device_split(const void* d_packed, const void* d_eq, int log_n, void* d_out,
                                                size_t max_blocks_per_group, void* stream) {
	if (int rc = rs_check(d_packed, d_eq, log_n, d_out)) return rc;
	BN_CHECK_ARG(is_aligned(d_packed, 16) && is_aligned(d_eq, 16) && is_aligned(d_out, 16), "device buffers must be 16-byte aligned");
	const uint64_t bytes = (uint64_t)16 << log_n;
	BN_CHECK_ARG(!ranges_overlap(d_packed, bytes, d_out, 128 * 16) && !ranges_overlap(d_eq, bytes, d_out, 128 * 16),
	             "d_out must not overlap an input");
	return rs_launch(d_packed, d_eq, log_n, d_out, max_blocks_per_group, (hipStream_t)stream);
}

extern "C" int bn_rs_partial_evals_device(const void* d_packed, const void* d_eq, int log_n, void* d_out, void* stream) {
	return bn_rs_partial_evals_device_split(d_packed, d_eq, log_n, d_out, 0, stream);
}

extern "C" int bn_rs_partial_evals_host(int device, const uint32_t* packed, const uint32_t* eq, int log_n, uint32_t* out) {
	if (int rc = rs_check(packed, eq, log_n, out)) return rc;
	BN_DEVICE_SCOPE(device);
	const size_t bytes = (size_t)16 << log_n;
	// staged per call, both columns and the result in one allocation: the size depends on log_n
	DevBuf buf;
	CallStream cs;
	if (int rc = buf.alloc(2 * bytes + 128 * 16)) return rc;
	if (int rc = cs.create()) return rc;
	void* d_eq = (char*)buf.p + bytes;
	void* d_dst = (char*)buf.p + 2 * bytes;
	return staged_call(cs.s, packed, buf.p, bytes, d_dst, out, 128 * 16, [&](hipStream_t st) -> int {
		BN_HIP(hipMemcpyAsync(d_eq, eq, bytes, hipMemcpyHostToDevice, st));
		return rs_launch(buf.p, d_eq, log_n, d_dst, 0, st);
	});
}

extern "C" int bn_gf128_linear_map_device(const void* d_in, void* d_out, size_t n, const uint32_t* matrix, int bitsliced,
                                          void* stream) {
	if (int rc = map_check(d_in, d_out, n, matrix, bitsliced)) return rc;
	BN_CHECK_ARG(is_aligned(d_in, 16) && is_aligned(d_out, 16), "device buffers must be 16-byte aligned");
	const uint64_t bytes = (uint64_t)n * (bitsliced ? 512 : 16);
	BN_CHECK_ARG(d_in == d_out || !ranges_overlap(d_in, bytes, d_out, bytes), "d_in and d_out must be the same buffer or not overlap");
	return map_launch(d_in, d_out, n, matrix, bitsliced, (hipStream_t)stream);
}

extern "C" int bn_gf128_linear_map_host(int device, const uint32_t* in, size_t n, const uint32_t* matrix, int bitsliced,
                                        uint32_t* out) {
	if (int rc = map_check(in, out, n, matrix, bitsliced)) return rc;
	BN_DEVICE_SCOPE(device);
	const size_t bytes = n * (bitsliced ? 512 : 16);
	DevBuf buf;  // staged per call, mapped in place: the size depends on n
	CallStream cs;
	if (int rc = buf.alloc(bytes)) return rc;
	if (int rc = cs.create()) return rc;
	return staged_call(cs.s, in, buf.p, bytes, buf.p, out, bytes,
	                   [&](hipStream_t st) { return map_launch(buf.p, buf.p, n, matrix, bitsliced, st); });
}
