// FRI-Binius codeword folding on the additive-NTT plan (GF(2^128) plans). No reference counterpart.
//
// Semantics: the codeword at round i is 2^log_rate blocks (coset-major) of m_i = 2^(log_h-i)
// compact elements; round 0 is bn_antt_forward_device's output. One round with challenge r undoes
// inverse-NTT stage i on every pair and combines the two halves:
//   u = in[c][2j], v = in[c][2j+1], t = twiddle(stage i, blk j, coset c)   (antt.hip)
//   v' = u ^ v ; u' = u ^ t*v' (limb-wise GF(2^32)) ; out[c][j] = u' ^ r*(u' ^ v')   (GF(2^128))
// An arity-k call runs rounds i .. i+k-1 (r_0 first) in one launch: the input is read once, the
// output written once, the levels in between stay in LDS.
//
// Indexing: batch, coset and j are consecutive in memory at every level, so with P the global index
// of a pair at level l (stage st = i + l) its twiddle index (coset << (log_h-1-st)) | blk is the low
// log_h + log_rate - 1 - st bits of P, and the level's output goes to position P.
//
//   antt_fold      a work-group takes tiles of kFoldTile consecutive input elements (2^(11-arity)
//                  chunks), grid-strided. Level 0 reads its pairs from global memory (32 B per lane,
//                  consecutive lanes consecutive pairs), levels 1.. read the previous level from LDS
//                  (two buffers taken in turn, one barrier per level), the last level writes global
//                  memory.
//
// Twiddles: the tile is aligned, so P = tile part | q (q the pair inside the tile) and the twiddle
// is the XOR of a work-group-uniform word (the bits of P above the lane's: scalar code, once per
// level and 512 pairs) and a per-thread word (the up to nine bits the thread index gives, once per
// thread and level). Nothing is built per pair from all log_h + log_rate bits.
//
// Products: t*v' is four table-leaf GF(2^32) products (dmul_t32<5>). x -> r*x is GF(2)-linear and r
// is a launch constant, so each work-group tabulates it once per level (gf128_rtab.hpp, shared with
// the eq-indicator expansion): r * (e << 4n) for the 32
// nibble positions n and the 16 nibble values e (8 KiB of LDS per level, built from 128 dmul128_t
// products of r with the unit elements), and a product is the XOR of 32 16-byte LDS reads. The 16
// entries of a nibble position are 256 consecutive bytes, one per bank group: lanes with equal
// nibbles read the same address, lanes with different nibbles different banks.
#include <hip/hip_runtime.h>

#include "antt_plan.hpp"
#include "field_dev.hpp"
#include "gf128_rtab.hpp"

namespace bn {

constexpr int kFoldTileLog = 11;  // input elements per tile: 32 KiB read, 16 + 8 KiB of LDS levels
constexpr int kFoldTile = 1 << kFoldTileLog;
constexpr int kFoldThreadsLog = 9;  // 8 waves: two work-groups a CU at up to 128 VGPRs share their tables of r
constexpr int kFoldThreads = 1 << kFoldThreadsLog;
constexpr int kFoldMaxArity = 8;
constexpr int kFoldRTab = kRTabEntries;                 // uint4 entries of one level's table of r (gf128_rtab.hpp)
constexpr int kFoldGf8 = (kGf8LdsBytes + 15) / 16;      // uint4 slots of the GF(2^8) tables
constexpr int kFoldWgsPerCu = 2;                        // resident work-groups (128 VGPRs, LDS up to arity 6)

// dynamic LDS: arity tables of r, the GF(2^8) tables, and for arity > 1 the two level buffers
static size_t fold_lds_bytes(int arity) {
	return 16 * ((size_t)arity * kFoldRTab + kFoldGf8 + (arity > 1 ? kFoldTile / 2 + kFoldTile / 4 : 0));
}

struct FoldParams {
	const uint4* src;
	uint4* dst;
	const uint32_t* s;  // subspace table, log_h x width
	int width;
	int nbits0;  // twiddle index bits of the first level: log_h + log_rate - 1 - round
	int round, arity;
	unsigned long long n_in;  // input elements in all (batch * 2^(log_h + log_rate - round))
	uint4 r[kFoldMaxArity];   // the challenges, by value
};

// XOR of row[b] over the set bits b in [lo, hi) of x
__device__ __forceinline__ uint32_t fold_tw_bits(const uint32_t* row, unsigned long long x, int lo, int hi) {
	uint32_t w = 0;
	for (int b = lo; b < hi; b++) w ^= ((x >> b) & 1) ? row[b] : 0u;
	return w;
}

// one pair: the inverse butterfly with twiddle t, then the two halves combined at r (table T)
__device__ __forceinline__ uint4 fold_pair(uint4 u, uint4 v, uint32_t t, const uint4* T, const uint8_t* tab) {
	v = xor4(v, u);
	u.x ^= dmul_t32<5>(t, v.x, tab);
	u.y ^= dmul_t32<5>(t, v.y, tab);
	u.z ^= dmul_t32<5>(t, v.z, tab);
	u.w ^= dmul_t32<5>(t, v.w, tab);
	return xor4(u, fold_mul_r(T, xor4(u, v)));
}

__global__ __launch_bounds__(kFoldThreads, kFoldWgsPerCu) void antt_fold(FoldParams P) {
	extern __shared__ uint4 fold_lds[];
	uint4* rtab = fold_lds;                                       // [arity][32][16]
	uint8_t* tab = (uint8_t*)(fold_lds + P.arity * kFoldRTab);   // GF(2^8) log/exp tables
	// level l's output: kFoldTile >> (l + 1) elements, even levels in buf0, odd levels in buf1
	uint4* buf0 = fold_lds + P.arity * kFoldRTab + kFoldGf8;
	uint4* buf1 = buf0 + kFoldTile / 2;
	constexpr int kSlots = kFoldTile / 2 / kFoldThreads;  // level-0 pairs per thread
	const int tid = threadIdx.x;

	// ---- the tables of r_0 .. r_{arity-1} (four levels at a time)
	gf8_tables_to_lds(tab);
	__syncthreads();
	fold_build_rtab<kFoldThreads>(rtab, P.arity, [&](int l, int j) {
		const uint32_t bit = 1u << (j & 31);
		const uint4 e = make_uint4((j >> 5) == 0 ? bit : 0u, (j >> 5) == 1 ? bit : 0u, (j >> 5) == 2 ? bit : 0u,
		                           (j >> 5) == 3 ? bit : 0u);
		return dmul128_t(e, P.r[l], tab);
	});

	const unsigned long long n_tiles = (P.n_in + kFoldTile - 1) >> kFoldTileLog;
	for (unsigned long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
		const unsigned long long tile0 = tile << kFoldTileLog;  // first input element

		// ---- level 0: pairs from global memory, every load of the thread in flight before the products
		{
			const unsigned long long pair0 = tile0 >> 1, n_pairs = P.n_in >> 1;
			uint4 u[kSlots], v[kSlots];
#pragma unroll
			for (int n = 0; n < kSlots; n++) {
				const unsigned long long pg = pair0 + (unsigned)(tid + n * kFoldThreads);
				if (pg < n_pairs) {
					u[n] = P.src[2 * pg];
					v[n] = P.src[2 * pg + 1];
				}
			}
			const int nbits = P.nbits0;
			const uint32_t* srow = P.s + (size_t)P.round * P.width;
			const uint32_t w_lane = fold_tw_bits(srow, (unsigned)tid, 0, nbits < kFoldThreadsLog ? nbits : kFoldThreadsLog);
#pragma unroll
			for (int n = 0; n < kSlots; n++) {
				const int q = tid + n * kFoldThreads;
				const unsigned long long pg = pair0 + (unsigned)q;
				if (pg < n_pairs) {
					// the bits above the lane's: uniform over the work-group
					const uint32_t w = w_lane ^ fold_tw_bits(srow, pair0 + (unsigned)(n * kFoldThreads), kFoldThreadsLog, nbits);
					const uint4 o = fold_pair(u[n], v[n], w, rtab, tab);
					if (P.arity == 1)
						P.dst[pg] = o;
					else
						buf0[q] = o;
				}
			}
		}

		// ---- levels 1 .. arity-1: pairs from the previous level's LDS buffer
#pragma unroll 1
		for (int l = 1; l < P.arity; l++) {
			__syncthreads();
			const int tile_log = kFoldTileLog - 1 - l;  // log2 of the tile's pairs of this level
			const int lane_bits = tile_log < kFoldThreadsLog ? tile_log : kFoldThreadsLog;
			const unsigned long long pair0 = tile0 >> (l + 1);    // the tile's first pair of this level
			const unsigned long long n_pairs = P.n_in >> (l + 1);  // pairs of this level in all
			const int nbits = P.nbits0 - l;
			const uint32_t* srow = P.s + (size_t)(P.round + l) * P.width;
			const uint32_t w_lane = fold_tw_bits(srow, (unsigned)tid, 0, nbits < lane_bits ? nbits : lane_bits);
			const uint4* rd = (l & 1) ? buf0 : buf1;  // level l - 1's output
			uint4* wr = (l & 1) ? buf1 : buf0;
			const uint4* T = rtab + l * kFoldRTab;
#pragma unroll 1
			for (int q0 = 0; q0 < (1 << tile_log); q0 += kFoldThreads) {
				const int q = q0 + tid;
				const unsigned long long pg = pair0 + (unsigned)q;
				if (q < (1 << tile_log) && pg < n_pairs) {
					const uint32_t w = w_lane ^ fold_tw_bits(srow, pair0 + (unsigned)q0, lane_bits, nbits);
					const uint4 o = fold_pair(rd[2 * q], rd[2 * q + 1], w, T, tab);
					if (l == P.arity - 1)
						P.dst[pg] = o;
					else
						wr[q] = o;
				}
			}
		}
		if (P.arity > 1) __syncthreads();  // the next tile's level 0 writes buf0
	}
}

// One launch: `batch` codewords of round `round` folded `arity` times. Arguments are checked by the caller.
int launch_fold(bn_antt_plan* plan, const void* d_in, void* d_out, int round, int arity, const uint32_t* challenges,
                size_t batch, hipStream_t st) {
	FoldParams prm;
	prm.src = (const uint4*)d_in;
	prm.dst = (uint4*)d_out;
	prm.s = plan->s_dev;
	prm.width = plan->width;
	prm.nbits0 = plan->log_h + plan->log_rate - 1 - round;
	prm.round = round;
	prm.arity = arity;
	prm.n_in = (unsigned long long)batch << (plan->log_h + plan->log_rate - round);
	for (int i = 0; i < kFoldMaxArity; i++) prm.r[i] = i < arity ? words4(challenges + 4 * i) : make_uint4(0, 0, 0, 0);
	// a tile holds whole chunks (2^arity <= kFoldTile) and the last one may be partly empty. One
	// work-group per tile up to what the device holds at once; beyond that the work-groups stride,
	// so the tables of r are built once per resident work-group (num_cus is known for log_h >= 12
	// plans; the others rarely reach the cap)
	const unsigned long long n_tiles = (prm.n_in + kFoldTile - 1) >> kFoldTileLog;
	const unsigned long long cap = (unsigned long long)(plan->num_cus > 0 ? plan->num_cus : 256) * kFoldWgsPerCu;
	const unsigned grid = (unsigned)(n_tiles < cap ? n_tiles : cap);
	// up to 90 KiB (arity 8), above the 64 KiB default: set before every launch (cheap, and
	// correct when the caller switches devices)
	BN_HIP(hipFuncSetAttribute((const void*)antt_fold, hipFuncAttributeMaxDynamicSharedMemorySize,
	                           (int)fold_lds_bytes(kFoldMaxArity)));
	void* args[] = {&prm};
	BN_HIP(hipLaunchKernel((const void*)antt_fold, dim3(grid), dim3(kFoldThreads), args, fold_lds_bytes(arity), st));
	return BN_OK;
}

}  // namespace bn

using namespace bn;

static int fold_check(const bn_antt_plan* p, int round, int arity, const uint32_t* challenges) {
	BN_CHECK_ARG(p != nullptr, "plan is NULL");
	BN_CHECK_ARG(challenges != nullptr, "challenges is NULL");
	if (p->field_bits != 128) BN_FAIL(BN_ERR_UNSUPPORTED, "the FRI fold is built for GF(2^128) plans (challenges live in GF(2^128))");
	BN_CHECK_ARG(round >= 0, "round must be >= 0 (got %d)", round);
	BN_CHECK_ARG(arity >= 1 && arity <= kFoldMaxArity, "arity must be in [1, %d] (got %d)", kFoldMaxArity, arity);
	BN_CHECK_ARG(round <= p->log_h && arity <= p->log_h - round, "round + arity must be <= log_h = %d (got %d + %d)", p->log_h,
	             round, arity);
	return BN_OK;
}

extern "C" int bn_antt_fri_fold_device(bn_antt_plan* p, const void* d_in, void* d_out, int round, int arity,
                                       const uint32_t* challenges, size_t batch, void* stream) {
	if (int rc = fold_check(p, round, arity, challenges)) return rc;
	if (int rc = check_device_args(p, d_in, d_out, batch)) return rc;
	const int log_in = p->log_h + p->log_rate - round;
	BN_CHECK_ARG(batch <= (((size_t)1 << 40) >> log_in), "batch of %zu codewords is too large", batch);
	const size_t in_bytes = (batch << log_in) * 16;
	BN_CHECK_IO_DISJOINT(d_in, in_bytes, d_out, in_bytes >> arity);
	BN_DEVICE_SCOPE(p->device);
	return launch_fold(p, d_in, d_out, round, arity, challenges, batch, (hipStream_t)stream);
}

extern "C" int bn_antt_fri_fold_host(bn_antt_plan* p, const void* in, size_t in_elems, int round, int arity,
                                     const uint32_t* challenges, void* out) {
	if (int rc = fold_check(p, round, arity, challenges)) return rc;
	BN_CHECK_ARG(in != nullptr && out != nullptr, "host buffers must be non-NULL");
	const int log_in = p->log_h + p->log_rate - round;
	BN_CHECK_ARG(in_elems == ((size_t)1 << log_in), "input has %zu elements, round %d of the plan has 2^%d", in_elems, round,
	             log_in);
	BN_DEVICE_SCOPE(p->device);
	const size_t in_bytes = in_elems * 16;
	const size_t out_bytes = in_bytes >> arity;
	if (!p->own_stream) BN_HIP(hipStreamCreateWithFlags(&p->own_stream, hipStreamNonBlocking));
	// staged per call, input and output in one allocation: a fold's sizes depend on the round
	DevBuf buf;
	if (int rc = buf.alloc(in_bytes + out_bytes)) return rc;
	void* d_dst = (char*)buf.p + in_bytes;
	return staged_call(p->own_stream, in, buf.p, in_bytes, d_dst, out, out_bytes,
	                   [&](hipStream_t st) { return launch_fold(p, buf.p, d_dst, round, arity, challenges, 1, st); });
}
