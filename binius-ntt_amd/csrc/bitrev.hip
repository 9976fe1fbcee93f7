// The bit-reversal permutation of a device-resident GF(2^128) column. No reference counterpart.
//
// Semantics: out[b*2^n + rev_n(x)] = in[b*2^n + x], x < 2^n, b < batch, compact 16-byte elements. It
// puts a coefficient column into the order in which the sumcheck (highest variable first) binds the
// variables the way the FRI fold (lowest index bit first) does.
//
// Tiles (bitrev_plan.hpp): the index is split hi (q) | mid (n - 2q) | lo (q), q = 6. A tile, one value
// of mid in one transform, is 2^12 elements (64 KiB of LDS, two work-groups a CU): read as 64 runs of
// 1 KiB, one per hi, written as 64 runs of 1 KiB, one per rev(lo). Every global access is whole
// 128-byte lines; done element by element the permutation moves 16-byte pieces 2^(n-q) * 16 B apart.
//
//   bit_reverse_tiles  a work-group of 512 threads takes tiles, grid-strided. A thread loads its eight
//                      elements of the tile (consecutive lanes consecutive elements of a run, all
//                      eight in flight), writes them to LDS as loaded (ds_write_b128), and after the
//                      barrier reads the transposed, reversed positions (rev from __brev) and stores
//                      them, consecutive lanes consecutive elements of an output run. The next tile's
//                      loads are issued between the barrier and the stores, so they fly under the
//                      LDS reads and the stores. The LDS column is XOR-swizzled with the row's four
//                      highest bits (bitrev_lds_slot): unswizzled, the transposed ds_read_b128 of rows
//                      0 mod 64 dwords apart is a 16-way bank conflict.
//
// log_n <= 1 is the identity: one device-to-device copy. Loads are non-temporal (every element is
// touched once); so are the stores of a compact result. Bitsliced output stores plainly and queues the
// in-place k_bitslice launch (field.hip) behind the permutation, as the eq expansion does.
#include <hip/hip_runtime.h>

#include "bitrev_plan.hpp"
#include "common.hpp"
#include "stream_io.hpp"

int bitslice_launch(const void* src, void* dst, size_t nblk, int untranspose, hipStream_t st);  // field.hip

namespace bn {

static_assert(kBitrevPerThread * kBitrevThreads == 1 << (2 * kBitrevTileLog), "a full tile is kBitrevPerThread elements a thread");
static_assert(2 * ((size_t)16 << (2 * kBitrevTileLog)) <= kBitrevLdsPerCu, "two full tiles a CU");

struct BitrevParams {
	const uint4* in;
	uint4* out;
	BitrevPlan plan;
	int stream_out;  // non-temporal stores (compact output)
};

__device__ __forceinline__ void bitrev_load(uint4 (&v)[kBitrevPerThread], const BitrevParams& P, unsigned long long tile, uint32_t elems) {
#pragma unroll
	for (int i = 0; i < kBitrevPerThread; i++) {
		const uint32_t e = (uint32_t)i * kBitrevThreads + threadIdx.x;
		if (e < elems) v[i] = ld_stream((const uint32_t*)(P.in + bitrev_in_index(P.plan, tile, e)));
	}
}

__global__ __launch_bounds__(kBitrevThreads) void bit_reverse_tiles(BitrevParams P) {
	extern __shared__ uint4 bitrev_lds[];
	const int q = P.plan.q;
	const uint32_t elems = bitrev_tile_elems(P.plan), lo_mask = (1u << q) - 1;
	uint4 v[kBitrevPerThread];

	unsigned long long tile = blockIdx.x;
	if (tile < P.plan.n_tiles) bitrev_load(v, P, tile, elems);
	for (; tile < P.plan.n_tiles; tile += gridDim.x) {
#pragma unroll
		for (int i = 0; i < kBitrevPerThread; i++) {
			const uint32_t e = (uint32_t)i * kBitrevThreads + threadIdx.x;
			if (e < elems) bitrev_lds[bitrev_lds_slot(q, e >> q, e & lo_mask)] = v[i];
		}
		__syncthreads();
		const unsigned long long next = tile + gridDim.x;
		if (next < P.plan.n_tiles) bitrev_load(v, P, next, elems);
#pragma unroll
		for (int i = 0; i < kBitrevPerThread; i++) {
			const uint32_t e = (uint32_t)i * kBitrevThreads + threadIdx.x;
			if (e < elems) {
				const uint4 w = bitrev_lds[bitrev_lds_read_slot(q, e)];
				uint4* dst = P.out + bitrev_out_index(P.plan, tile, e);
				if (P.stream_out)
					st_stream((uint32_t*)dst, w);
				else
					*dst = w;
			}
		}
		__syncthreads();  // the next tile's rows overwrite the slots just read
	}
}

// The permutation on `st`, then the bit transpose. Arguments are checked by the caller; the current
// device is the buffers'.
static int bitrev_launch(const BitrevPlan& plan, size_t batch, const void* d_in, void* d_out, int bitsliced, hipStream_t st) {
	const size_t n_elems = batch << plan.n;
	if (plan.n <= 1) {
		BN_HIP(hipMemcpyAsync(d_out, d_in, n_elems * 16, hipMemcpyDeviceToDevice, st));
	} else {
		int dev = 0, num_cus = 0;
		BN_HIP(hipGetDevice(&dev));
		BN_HIP(hipDeviceGetAttribute(&num_cus, hipDeviceAttributeMultiprocessorCount, dev));
		BN_HIP(hipFuncSetAttribute((const void*)bit_reverse_tiles, hipFuncAttributeMaxDynamicSharedMemorySize,
		                           (int)bitrev_lds_bytes(kBitrevTileLog)));
		BitrevParams prm;
		prm.in = (const uint4*)d_in;
		prm.out = (uint4*)d_out;
		prm.plan = plan;
		prm.stream_out = !bitsliced;
		const unsigned grid = (unsigned)bitrev_grid(plan, num_cus);
		void* args[] = {&prm};
		BN_HIP(hipLaunchKernel((const void*)bit_reverse_tiles, dim3(grid), dim3(kBitrevThreads), args, bitrev_lds_bytes(plan.q), st));
	}
	if (bitsliced) return bitslice_launch(d_out, d_out, n_elems >> 5, 0, st);
	return BN_OK;
}

static int bitrev_check(const void* in, const void* out, int log_n, size_t batch, int bitsliced, int tile_log, BitrevPlan* plan) {
	BN_CHECK_ARG(in != nullptr && out != nullptr, "NULL buffer");
	BN_CHECK_ARG(log_n >= 0 && log_n <= kBitrevMaxLog, "log_n must be in [0, %d] (got %d)", kBitrevMaxLog, log_n);
	BN_CHECK_ARG(!bitsliced || log_n >= 5, "bitsliced output needs log_n >= 5 (got %d)", log_n);
	BN_CHECK_ARG(tile_log >= 0 && tile_log <= kBitrevTileLog, "tile_log must be in [0, %d] (got %d)", kBitrevTileLog, tile_log);
	BN_CHECK_ARG(batch != 0, "batch must be >= 1");
	BN_CHECK_ARG(bitrev_plan(log_n, batch, tile_log, plan), "batch of %zu transforms of 2^%d elements is above 2^32 elements", batch,
	             log_n);
	return BN_OK;
}

}  // namespace bn

using namespace bn;

extern "C" int bn_bit_reverse_device_split(const void* d_in, void* d_out, int log_n, size_t batch, int bitsliced, int tile_log,
                                           void* stream) {
	BitrevPlan plan;
	if (int rc = bitrev_check(d_in, d_out, log_n, batch, bitsliced, tile_log, &plan)) return rc;
	BN_CHECK_ARG(is_aligned(d_in, 16) && is_aligned(d_out, 16), "device buffers must be 16-byte aligned");
	const uint64_t bytes = ((uint64_t)batch << log_n) * 16;
	BN_CHECK_IO_DISJOINT(d_in, bytes, d_out, bytes);
	return bitrev_launch(plan, batch, d_in, d_out, bitsliced, (hipStream_t)stream);
}

extern "C" int bn_bit_reverse_device(const void* d_in, void* d_out, int log_n, size_t batch, int bitsliced, void* stream) {
	return bn_bit_reverse_device_split(d_in, d_out, log_n, batch, bitsliced, 0, stream);
}

extern "C" int bn_bit_reverse_host(int device, const uint32_t* in, int log_n, int bitsliced, uint32_t* out) {
	BitrevPlan plan;
	if (int rc = bitrev_check(in, out, log_n, 1, bitsliced, 0, &plan)) return rc;
	BN_DEVICE_SCOPE(device);
	const size_t bytes = (size_t)16 << log_n;
	// staged per call, input and output in one allocation: the size depends on log_n
	DevBuf buf;
	CallStream cs;
	if (int rc = buf.alloc(2 * bytes)) return rc;
	if (int rc = cs.create()) return rc;
	void* d_dst = (char*)buf.p + bytes;
	return staged_call(cs.s, in, buf.p, bytes, d_dst, out, bytes,
	                   [&](hipStream_t st) { return bitrev_launch(plan, 1, buf.p, d_dst, bitsliced, st); });
}
