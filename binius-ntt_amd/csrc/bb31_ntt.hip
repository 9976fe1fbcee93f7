// BabyBear (p = 15 * 2^27 + 1) NTT for gfx950: the prime-field sibling of the additive NTT
// (SURVEY.md §8f row 4). Replaces NTT<BB31> of the reference (src/ulvt/ntt/gpuntt.cuh:126-209):
// the reference bit-reverses the input and runs log_n radix-2 stages with bit-reversed
// twiddles, 11 stages per launch; its output is the natural-order DFT
//     X[k] = sum_j x[j] w^(j k),   w = g^(2^(log_group - log_n))
// (checked against the oracle and the reference's MD5 table, tests/golden/bb31_ntt_md5.json).
//
// MI355X design: a mixed-radix "four-step" decomposition with natural order in and out, so
// there is no bit-reversal pass at all. log_n = m_1 + ... + m_L bits (m_i <= 9, L = 1 for
// log_n <= 13). Pass p views the current sub-problem of size M_{p-1} = 2^{m_p} * M_p as
// rows j_p (stride M_p) x columns (the lower digits, contiguous):
//     Y[k_p][c] = DFT_{2^{m_p}} over j_p of Z[j_p][c],   then  Y[k_p][c] *= w_{M_{p-1}}^(c k_p)
// and stores Y in place (row k_p). The last pass takes 32 consecutive k_1 per tile, so both its
// reads (runs of 2^{m_L}) and its writes of the natural-order output X[k_1 + N_1 k_2 + ...]
// (runs of 32 k_1) are coalesced. A tile (2^{m_p} rows x 32 columns, <= 64 KiB) is one
// workgroup; its DFT runs as radix-2 DIF stages in LDS. Values are canonical u32 (< p) in HBM;
// products are Montgomery multiplications by Montgomery-encoded twiddles (risc0_baby_bear.h
// mul, lines 172-180, so w * R is stored). A bit-reversed input (DataOrder::BIT_REVERSED) is
// read through the first pass's addressing: the reads stay runs of 2^{m_1} words.
// The digit split, the pass tables, the twiddle table and the launch of every pass are planned on
// the host (bb31_plan.cpp); this file holds the kernels and launches what the planner says.
#include <hip/hip_runtime.h>

#include "bb31_plan.hpp"
#include "common.hpp"

struct bn_bb31_ntt_plan {
	int device = 0;
	bn::bb31::BbPlan plan{};   // the passes, built once
	uint32_t* wtab = nullptr;  // bb_twiddles: Montgomery-encoded w^e
	uint32_t* scratch = nullptr;  // passes 1..L-1 run in place here: n * batch words, grown on demand
	size_t scratch_words = 0;
	hipStream_t own_stream = nullptr;
	uint32_t* h_dev = nullptr;  // host-apply staging (in, out)
};

namespace bn {
namespace {
using namespace bb31;

constexpr uint32_t kPinv = 0x88000001u;  // p^-1 mod 2^32 (risc0::Fp::M)

__host__ __device__ inline uint32_t mont(uint32_t a, uint32_t b) {
	uint64_t o = (uint64_t)a * b;
	const uint32_t red = (0u - (uint32_t)o) * kPinv;
	o += (uint64_t)red * kP;
	const uint32_t r = (uint32_t)(o >> 32);
	return r >= kP ? r - kP : r;
}
__host__ __device__ inline uint32_t bb_add(uint32_t a, uint32_t b) {
	const uint32_t r = a + b;
	return r >= kP ? r - kP : r;
}
__host__ __device__ inline uint32_t bb_sub(uint32_t a, uint32_t b) { return a >= b ? a - b : a + kP - b; }
__host__ __device__ inline uint32_t bb_reduce(uint32_t x) {  // any u32 -> canonical (BB31(r) == r mod p)
	x = x >= kP ? x - kP : x;
	return x >= kP ? x - kP : x;
}

struct BbArgs {
	const uint32_t* src;
	uint32_t* dst;
	const uint32_t* wtab;
	size_t n;  // words per transform
	int log_n;
	int hi_split;  // 1: wtab = lo[4096] ++ hi[]
	BbPass p;
};

// w^e for e < 2^log_n, Montgomery-encoded
__device__ inline uint32_t wpow(const BbArgs& A, uint32_t e) {
	if (!A.hi_split) return A.wtab[e];
	return mont(A.wtab[e & ((1u << kLoBits) - 1)], A.wtab[(1u << kLoBits) + (e >> kLoBits)]);
}

__device__ inline uint32_t rev_bits(uint32_t v, int bits) { return bits ? __brev(v) >> (32 - bits) : 0u; }

// The single-tile kernel (role 2, log_n <= kMaxSingleM): the whole transform is one column of
// R = 2^m rows in LDS, row r at lds[r]; behind it the tile DFT's twiddles w_R^i (Montgomery-encoded),
// i < R/2 (bb_lds_bytes).
__global__ __launch_bounds__(kThreads) void bb_pass(BbArgs A) {
	extern __shared__ uint32_t lds[];
	const BbPass& ps = A.p;
	const int m = ps.m;
	const int R = 1 << m;
	const int tid = threadIdx.x;
	const size_t b = blockIdx.y;  // transform of the batch
	const uint32_t* src = A.src + b * A.n;
	uint32_t* dst = A.dst + b * A.n;
	uint32_t* twl = lds + R;
	for (int i = tid; i < R / 2; i += kThreads) twl[i] = wpow(A, (uint32_t)i << (A.log_n - m));
	for (int r = tid; r < R; r += kThreads)
		lds[r] = bb_reduce(src[ps.bitrev_in ? (size_t)rev_bits((uint32_t)r, A.log_n) : (size_t)r]);
	__syncthreads();
	// radix-2 DIF stages: natural-order rows in, bit-reversed rows out; stage st uses
	// w_{2 half}^k = w_R^(k R / (2 half))
	for (int st = m - 1; st >= 0; st--) {
		const int half = 1 << st;
		for (int pr = tid; pr < R / 2; pr += kThreads) {
			const int k = pr & (half - 1);
			const int r0 = ((pr >> st) << (st + 1)) | k;
			uint32_t* pu = lds + r0;
			uint32_t* pv = pu + half;
			const uint32_t x = *pu, y = *pv;
			*pu = bb_add(x, y);
			const uint32_t d = bb_sub(x, y);
			*pv = k ? mont(d, twl[k << (m - 1 - st)]) : d;
		}
		__syncthreads();
	}
	for (int k = tid; k < R; k += kThreads) dst[k] = lds[rev_bits((uint32_t)k, m)];  // row k is held at LDS row rev_m(k)
}

// The multi-pass roles (0 first/middle, 1 last), M = m in [kMinM, kMaxM]: a tile of R = 2^M rows x
// kCols columns, register-resident. A thread holds E = R/8 elements of one column, rows
// t + 8i, so the radix-2 stages with half >= 8 run in registers; one LDS exchange regroups the
// column into runs of 8 rows for the last three stages. LDS traffic per tile: the exchange and the
// output gather. LDS: row r, column c at r * kCols + c (a row of 32 words spans half the banks),
// the tile DFT's twiddles behind the tile as in bb_pass.
template <int ROLE, int M>
__global__ __launch_bounds__(kThreads) void bb_pass_r(BbArgs A) {
	constexpr int R = 1 << M, E = R / 8;
	extern __shared__ uint32_t lds[];
	const BbPass& ps = A.p;
	const int tid = threadIdx.x;
	const size_t b = blockIdx.y;
	const uint32_t* src = A.src + b * A.n;
	uint32_t* dst = A.dst + b * A.n;
	const size_t tile = blockIdx.x;
	size_t q = 0, cb = 0, kb = 0, gpos = 0, gout = 0;
	if (ROLE == 0) {
		const size_t ncb = ((size_t)1 << ps.log_mp) / kCols;
		q = tile / ncb;
		cb = tile % ncb;
	} else {
		const size_t nkb = ((size_t)1 << ps.m1) / kCols;
		size_t g = tile / nkb;
		kb = tile % nkb;
		for (int i = 0; i < ps.ndig; i++) {
			const size_t d = g & (((size_t)1 << ps.mdig[i]) - 1);
			g >>= ps.mdig[i];
			gpos += d << ps.log_pos[i];
			gout += d << ps.log_out[i];
		}
	}
	// ROLE 0 reads rows of 32 contiguous columns (lanes along c); ROLE 1's rows are contiguous,
	// so 8 lanes walk 8 consecutive rows of one column
	const int c = ROLE == 0 ? tid % kCols : tid / 8;
	const int t = ROLE == 0 ? tid / kCols : tid % 8;
	auto src_addr = [&](int r) -> size_t {
		if (ROLE == 0) {
			const size_t j = (q << ps.log_sub) + ((size_t)r << ps.log_mp) + cb * kCols + c;
			return ps.bitrev_in ? (size_t)rev_bits((uint32_t)j, A.log_n) : j;
		}
		return ((kb * kCols + c) << (A.log_n - ps.m1)) + gpos + r;
	};
	uint32_t* twl = lds + R * kCols;
	for (int i = tid; i < R / 2; i += kThreads) twl[i] = wpow(A, (uint32_t)i << (A.log_n - M));
	uint32_t x[E];
#pragma unroll
	for (int i = 0; i < E; i++) x[i] = bb_reduce(src[src_addr(t + 8 * i)]);
	__syncthreads();  // twl
	// stages half = 2^s >= 8: rows t + 8i and t + 8i + half are both in this thread (i + half/8)
#pragma unroll
	for (int s = M - 1; s >= 3; s--) {
		const int hi = 1 << (s - 3);
#pragma unroll
		for (int i = 0; i < E; i++) {
			if (i & hi) continue;
			const uint32_t u = x[i], v = x[i + hi];
			const int k = (t + 8 * i) & ((1 << s) - 1);
			x[i] = bb_add(u, v);
			const uint32_t d = bb_sub(u, v);
			x[i + hi] = k ? mont(d, twl[k << (M - 1 - s)]) : d;
		}
	}
	// regroup: this thread takes rows 8g + j (j < 8) for g = t + 8u
#pragma unroll
	for (int i = 0; i < E; i++) lds[(t + 8 * i) * kCols + c] = x[i];
	__syncthreads();
#pragma unroll
	for (int u = 0; u < E / 8; u++)
#pragma unroll
		for (int j = 0; j < 8; j++) x[8 * u + j] = lds[(8 * (t + 8 * u) + j) * kCols + c];
#pragma unroll
	for (int s = 2; s >= 0; s--) {
		const int half = 1 << s;
#pragma unroll
		for (int i = 0; i < E; i++) {
			const int j = i & 7;
			if (j & half) continue;
			const uint32_t u = x[i], v = x[i + half];
			const int k = j & (half - 1);
			x[i] = bb_add(u, v);
			const uint32_t d = bb_sub(u, v);
			x[i + half] = k ? mont(d, twl[k << (M - 1 - s)]) : d;
		}
	}
#pragma unroll
	for (int u = 0; u < E / 8; u++)
#pragma unroll
		for (int j = 0; j < 8; j++) lds[(8 * (t + 8 * u) + j) * kCols + c] = x[8 * u + j];
	__syncthreads();
	// write row k (held at LDS row rev_M(k)). ROLE 0: inter-pass twiddle w_{M_{p-1}}^(c k); a
	// lane keeps its column and walks rows k = k0, k0 + 8, ... so the twiddle advances by one
	// Montgomery product per element from two table lookups per lane.
	if (ROLE == 0) {
		const int cc = tid % kCols, k0 = tid / kCols;
		const size_t cf = cb * kCols + cc;
		const size_t msk = ((size_t)1 << ps.log_sub) - 1;
		const int sh = A.log_n - ps.log_sub;
		uint32_t tw = wpow(A, (uint32_t)(((cf * (size_t)k0) & msk) << sh));
		const uint32_t step = wpow(A, (uint32_t)(((cf * (size_t)(kThreads / kCols)) & msk) << sh));
#pragma unroll 4
		for (int k = k0; k < R; k += kThreads / kCols) {
			const uint32_t v = mont(lds[rev_bits((uint32_t)k, M) * kCols + cc], tw);
			dst[(q << ps.log_sub) + ((size_t)k << ps.log_mp) + cf] = v;
			tw = mont(tw, step);
		}
	} else {
#pragma unroll 4
		for (int u = tid; u < R * kCols; u += kThreads) {
			const int k = u / kCols, cc = u % kCols;
			dst[(kb * kCols + cc) + gout + ((size_t)k << (A.log_n - M))] = lds[rev_bits((uint32_t)k, M) * kCols + cc];
		}
	}
}

// entry I of kBbInstances as a kernel
template <int I>
struct BbAt {
	static const void* fn() {
		constexpr BbInstance k = kBbInstances[I];
		if constexpr (k.role == BB_SINGLE) return (const void*)bb_pass;
		else return (const void*)bb_pass_r<k.role, k.m>;
	}
};
const void* bb_kernel_fn(int instance) { return instance_table<BbAt>(instance, std::make_index_sequence<kBbInstanceCount>()); }

// the device side of a new plan: the twiddle table, and the LDS attribute of every instance
int bb_plan_to_device(bn_bb31_ntt_plan* P, const std::vector<uint32_t>& tab) {
	BN_DEVICE_SCOPE(P->device);
	if (int rc = dev_alloc(&P->wtab, tab.size() * sizeof(uint32_t))) return rc;
	BN_HIP(hipMemcpy(P->wtab, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
	for (int i = 0; i < kBbInstanceCount; i++)
		BN_HIP(hipFuncSetAttribute(bb_kernel_fn(i), hipFuncAttributeMaxDynamicSharedMemorySize,
		                           (int)bb_lds_bytes(kBbInstances[i].role, kBbInstances[i].m)));
	return BN_OK;
}

// the scratch buffer at `words` words or more: grown on demand, freed with the plan
int bb_scratch(bn_bb31_ntt_plan* P, size_t words) {
	if (P->scratch_words >= words) return BN_OK;
	if (P->scratch) BN_HIP(hipFree(P->scratch));
	P->scratch = nullptr;
	P->scratch_words = 0;
	if (int rc = dev_alloc(&P->scratch, words * sizeof(uint32_t))) return rc;
	P->scratch_words = words;
	return BN_OK;
}

int bb_forward(bn_bb31_ntt_plan* P, const uint32_t* d_in, uint32_t* d_out, size_t batch, int bitrev, hipStream_t st) {
	const BbPlan& pl = P->plan;
	BbArgs A;
	A.wtab = P->wtab;
	A.n = (size_t)1 << P->plan.log_n;
	A.log_n = P->plan.log_n;
	A.hi_split = bb_hi_split(P->plan.log_n);
	// passes 1..L-1 run in place on a scratch buffer (first pass: in -> scratch), the last pass
	// scatters scratch -> out (its reads and writes are different index sets)
	uint32_t* work = d_out;
	if (pl.n_passes > 1) {
		if (int rc = bb_scratch(P, A.n * batch)) return rc;
		work = P->scratch;
	}
	for (int i = 0; i < pl.n_passes; i++) {
		A.src = i == 0 ? d_in : work;
		A.dst = i + 1 == pl.n_passes ? d_out : work;
		A.p = pl.pass[i];
		if (i == 0) A.p.bitrev_in = bitrev != 0;
		const BbLaunch l = bb_plan_launch(A.p, P->plan.log_n, batch);
		if (l.instance < 0) BN_FAIL(BN_ERR_UNSUPPORTED, "no kernel instance for role %d, m %d", A.p.role, A.p.m);
		void* args[] = {&A};
		BN_HIP(hipLaunchKernel(bb_kernel_fn(l.instance), dim3((unsigned)l.tiles, (unsigned)l.batch), dim3(l.threads), args, l.lds, st));
	}
	return BN_OK;
}

}  // namespace
}  // namespace bn

using namespace bn;

extern "C" int bn_bb31_ntt_plan_create(int device, uint32_t generator, int log_group_order, int log_n,
                                       bn_bb31_ntt_plan** out) {
	BN_CHECK_ARG(out != nullptr, "out is NULL");
	// NTTConfRad2 asserts (src/ulvt/ntt/nttconf.cuh:31-38)
	BN_CHECK_ARG(log_n >= 1 && log_n <= kMaxLogN, "log_n must be in [1, 27] (got %d)", log_n);
	BN_CHECK_ARG(log_group_order >= log_n && log_group_order <= kMaxLogN, "log_group_order must be in [log_n, 27]");
	int ndev = 0;
	BN_HIP(hipGetDeviceCount(&ndev));
	BN_CHECK_ARG(device >= 0 && device < ndev, "device %d out of range", device);
	auto* P = new bn_bb31_ntt_plan();
	P->device = device;
	bb_plan(log_n, &P->plan);
	if (const int rc = bb_plan_to_device(P, bb_twiddles(generator, log_group_order, log_n))) {
		bn_bb31_ntt_plan_destroy(P);
		return rc;
	}
	*out = P;
	return BN_OK;
}

extern "C" int bn_bb31_ntt_plan_destroy(bn_bb31_ntt_plan* P) {
	if (!P) return BN_OK;
	DeviceScope ds(P->device);
	if (P->wtab) (void)hipFree(P->wtab);
	if (P->scratch) (void)hipFree(P->scratch);
	if (P->h_dev) (void)hipFree(P->h_dev);
	if (P->own_stream) (void)hipStreamDestroy(P->own_stream);
	delete P;
	return BN_OK;
}

extern "C" int bn_bb31_ntt_forward_device(bn_bb31_ntt_plan* P, const uint32_t* d_in, uint32_t* d_out, size_t batch,
                                          int in_bit_reversed, void* stream) {
	BN_CHECK_ARG(P != nullptr, "plan is NULL");
	BN_CHECK_ARG(d_in != nullptr && d_out != nullptr, "device buffers must be non-NULL");
	BN_CHECK_ARG(batch >= 1 && batch <= 65535, "batch must be in [1, 65535]");
	const size_t bytes = ((size_t)4 << P->plan.log_n) * batch;
	BN_CHECK_IO_DISJOINT(d_in, bytes, d_out, bytes);
	BN_DEVICE_SCOPE(P->device);
	return bb_forward(P, d_in, d_out, batch, in_bit_reversed, (hipStream_t)stream);
}

// NTT<BB31>::apply (gpuntt.cuh:150-183): host in -> host out, synchronous; the input order
// flag replaces NTTData::order (BIT_REVERSED input is used as is, IN_ORDER is reversed first).
extern "C" int bn_bb31_ntt_forward_host(bn_bb31_ntt_plan* P, const uint32_t* in, size_t in_elems, uint32_t* out,
                                        int in_bit_reversed) {
	BN_CHECK_ARG(P != nullptr, "plan is NULL");
	BN_CHECK_ARG(in != nullptr && out != nullptr, "host buffers must be non-NULL");
	const size_t n = (size_t)1 << P->plan.log_n;
	BN_CHECK_ARG(in_elems == n, "input has %zu elements, plan expects 2^%d", in_elems, P->plan.log_n);
	BN_DEVICE_SCOPE(P->device);
	if (!P->h_dev)
		if (int rc = dev_alloc(&P->h_dev, 2 * n * sizeof(uint32_t))) return rc;
	if (!P->own_stream) BN_HIP(hipStreamCreateWithFlags(&P->own_stream, hipStreamNonBlocking));
	return staged_call(P->own_stream, in, P->h_dev, n * 4, P->h_dev + n, out, n * 4,
	                   [&](hipStream_t st) { return bb_forward(P, P->h_dev, P->h_dev + n, 1, in_bit_reversed, st); });
}
