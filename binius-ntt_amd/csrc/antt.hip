// Additive NTT over GF(2^32) / GF(2^128): plan management, C-ABI entry points and the
// v0 (correctness-first, compact-layout) kernel of both directions. The bitsliced fast path lives
// in antt_bs.hip (forward) and antt_inv.hip (inverse) and is selected when it supports the plan.
//
// Semantics (src/ulvt/ntt/additive_ntt.cuh): for each coset c < 2^log_rate the input is
// copied and butterflies u += w v ; v += u run for stage = log_h-1 .. 0 over blocks of
// 2^(stage+1) elements, with twiddle w = XOR_k s[stage][k] over the set bits k of
// (c << (log_h-1-stage)) | blk (calculate_twiddle, :59-77). Output is coset-major.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <cxxabi.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "antt_bs.hpp"
#include "field_dev.hpp"
#include "tower.hpp"

namespace bn {

// ------------------------------------------------------------------------------------
// v0 kernel: one launch per group of up to kTileLog stages. A workgroup owns a tile of
// 2^(k+c) elements: the k group bits [lo, lo+k) plus the c lowest index bits (so that
// each group of 2^c consecutive elements is read contiguously). Elements are staged in
// LDS; each thread walks its butterflies stage by stage.
// Both directions (INV: the inverse transform, antt_inv.hip): the forward runs the stages of a
// group downward over every coset block of the output; the inverse runs them upward with the
// butterfly undone (v += u ; u += w v, the same twiddle) over the one coset block it is given.
// ------------------------------------------------------------------------------------
constexpr int kTileLog = 12;  // 4096 elements; 64 KiB at 16 B/element

struct V0Params {
	const uint32_t* src;  // the caller's input (the forward's is shared by every coset)
	uint32_t* dst;        // d_out
	const uint32_t* s;    // subspace table, log_h x width
	int width;
	int log_h;
	int log_rate;
	int lo, k, c;
	int first;  // 1: the first group of the transform reads src, every other runs in place in dst
	int coset;  // inverse: the coset of the input block (the forward takes it from the block index)
};

template <int L, bool INV>
__global__ __launch_bounds__(256) void antt_v0_group(V0Params p) {
	extern __shared__ uint32_t lds[];
	const int tile_log = p.k + p.c;
	const int tile = 1 << tile_log;
	const int outer_log = p.log_h - tile_log;
	const size_t n = (size_t)1 << p.log_h;
	const int coset = INV ? p.coset : (int)(blockIdx.x >> outer_log);
	const size_t rest = INV ? blockIdx.x : blockIdx.x & (((size_t)1 << outer_log) - 1);
	const int mid_bits = p.lo - p.c;
	const size_t o_mid = rest & (((size_t)1 << mid_bits) - 1);
	const size_t o_hi = rest >> mid_bits;
	auto gidx = [&](int pos) -> size_t {
		const size_t cc = (size_t)pos & (((size_t)1 << p.c) - 1);
		const size_t g = (size_t)pos >> p.c;
		return (o_hi << (p.lo + p.k)) | (g << p.lo) | (o_mid << p.c) | cc;
	};
	uint32_t* dst = INV ? p.dst : p.dst + (size_t)coset * n * L;
	const uint32_t* src = p.first ? p.src : dst;

	uint8_t* tab = (uint8_t*)(lds + (size_t)tile * L);  // GF(2^8) log/exp tables after the tile
	gf8_tables_to_lds(tab);
	for (int pos = threadIdx.x; pos < tile; pos += blockDim.x) {
		const size_t gi = gidx(pos);
#pragma unroll
		for (int l = 0; l < L; l++) lds[pos * L + l] = src[gi * L + l];
	}
	__syncthreads();

	for (int i = 0; i < p.k; i++) {
		const int stage = INV ? p.lo + i : p.lo + p.k - 1 - i;
		const int b = stage - p.lo + p.c;
		const int npairs = tile >> 1;
		const uint32_t* srow = p.s + (size_t)stage * p.width;
		const int nbits = p.log_h + p.log_rate - 1 - stage;
		for (int q = threadIdx.x; q < npairs; q += blockDim.x) {
			const int pu = ((q >> b) << (b + 1)) | (q & ((1 << b) - 1));
			const int pv = pu | (1 << b);
			const size_t blk = gidx(pu) >> (stage + 1);
			const uint64_t ind = ((uint64_t)coset << (p.log_h - 1 - stage)) | (uint64_t)blk;
			uint32_t w = 0;
			for (int kk = 0; kk < nbits; kk++)
				if ((ind >> kk) & 1) w ^= srow[kk];
#pragma unroll
			for (int l = 0; l < L; l++) {
				uint32_t u = lds[pu * L + l], v = lds[pv * L + l];
				if (INV) v ^= u;
				u ^= (uint32_t)dmul_t<5>(w, v, tab);
				if (!INV) v ^= u;
				lds[pu * L + l] = u;
				lds[pv * L + l] = v;
			}
		}
		__syncthreads();
	}

	for (int pos = threadIdx.x; pos < tile; pos += blockDim.x) {
		const size_t gi = gidx(pos);
#pragma unroll
		for (int l = 0; l < L; l++) dst[gi * L + l] = lds[pos * L + l];
	}
}

// Optional per-launch hipEvent timing (bench.py): events are recorded on the launch stream
// around each kernel and resolved later (timing_resolve), so timing does not serialise the
// passes; `kind` identifies the pass.
static int timing_event(bn_antt_plan* p, hipEvent_t* e) {
	if (!p->ev_pool.empty()) {
		*e = p->ev_pool.back();
		p->ev_pool.pop_back();
		return BN_OK;
	}
	BN_HIP(hipEventCreate(e));
	return BN_OK;
}
int timing_begin(bn_antt_plan* p, int kind, hipStream_t st) {
	if (!p->timing) return BN_OK;
	(void)kind;
	int rc = timing_event(p, &p->cur_begin);
	if (rc != BN_OK) return rc;
	BN_HIP(hipEventRecord(p->cur_begin, st));
	return BN_OK;
}
int timing_end(bn_antt_plan* p, int kind, hipStream_t st) {
	if (!p->timing) return BN_OK;
	hipEvent_t e;
	int rc = timing_event(p, &e);
	if (rc != BN_OK) return rc;
	BN_HIP(hipEventRecord(e, st));
	p->pending.push_back({kind, p->cur_begin, e});
	return BN_OK;
}
static int timing_resolve(bn_antt_plan* p) {
	for (const auto& q : p->pending) {
		BN_HIP(hipEventSynchronize(q.end));
		float ms = 0.f;
		BN_HIP(hipEventElapsedTime(&ms, q.begin, q.end));
		if ((int)p->kind_ms.size() < q.kind + 1) {
			p->kind_ms.resize(q.kind + 1, 0.f);
			p->kind_cnt.resize(q.kind + 1, 0);
		}
		p->kind_ms[q.kind] += ms;
		p->kind_cnt[q.kind] += 1;
		p->ev_pool.push_back(q.begin);
		p->ev_pool.push_back(q.end);
	}
	p->pending.clear();
	return BN_OK;
}

// One transform on the compact kernel. The groups are balanced (an unbalanced tail would launch
// 2-point tiles): the forward takes them from the top stages down, the inverse the same list reversed.
static int launch_v0(bn_antt_plan* plan, const uint32_t* d_in, uint32_t* d_out, bool inv, int coset, hipStream_t st) {
	const int log_h = plan->log_h;
	const int L = plan->limbs;
	const int passes = (log_h + kTileLog - 1) / kTileLog;
	std::vector<std::pair<int, int>> groups;  // (lo, k)
	for (int hi = log_h, i = 0; hi > 0; i++) {
		const int k = (hi + (passes - i) - 1) / (passes - i);
		groups.push_back({hi - k, k});
		hi -= k;
	}
	if (inv) std::reverse(groups.begin(), groups.end());
	const void* fn = L == 4 ? (inv ? (const void*)antt_v0_group<4, true> : (const void*)antt_v0_group<4, false>)
	                        : (inv ? (const void*)antt_v0_group<1, true> : (const void*)antt_v0_group<1, false>);
	for (size_t i = 0; i < groups.size(); i++) {
		const int lo = groups[i].first, k = groups[i].second;
		const int c = std::min(lo, kTileLog - k);
		V0Params p{d_in, d_out, plan->s_dev, plan->width, log_h, plan->log_rate, lo, k, c, i == 0 ? 1 : 0, coset};
		// the forward writes every coset block, the inverse one block of n elements
		const size_t blocks = ((size_t)1 << (log_h - k - c)) << (inv ? 0 : plan->log_rate);
		const size_t lds = ((size_t)1 << (k + c)) * L * sizeof(uint32_t) + kGf8LdsBytes;
		BN_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
		// per-launch timing is the forward's (bench.py)
		int rc = inv ? BN_OK : timing_begin(plan, (int)i, st);
		if (rc != BN_OK) return rc;
		void* args[] = {&p};
		BN_HIP(hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(256), args, lds, st));
		rc = inv ? BN_OK : timing_end(plan, (int)i, st);
		if (rc != BN_OK) return rc;
	}
	return BN_OK;
}

const void* ntt_kernel_fn(int instance) {
	const NttFamily f = kNttInstances[instance].family;
	return f == NttFamily::Rr ? rr_kernel_fn(instance) : f == NttFamily::InvBs ? inv_kernel_fn(instance) : bs_kernel_fn(instance);
}

// A plan's setup for the bitsliced fast path (bs_supports), on creation and on the first change from variant 0
static int bs_prepare(bn_antt_plan* plan) {
	for (int i = 0; i < kNttInstanceCount; i++)
		BN_HIP(hipFuncSetAttribute(ntt_kernel_fn(i), hipFuncAttributeMaxDynamicSharedMemorySize, (int)instance_lds_bytes(kNttInstances[i])));
	// the pass tables are built here, once per plan, so that a table the kernels cannot run (a bottom
	// tile that is not one contiguous run, stage bits that are not the top tile bits) fails the plan
	// and never reaches a launch
	int rc = plan_pass_tables(plan->log_h, plan->log_rate, plan->s_host, plan->passes, plan->rt);
	if (rc != BN_OK) return rc;
	std::vector<uint32_t> ut;
	rc = plan_tile_starts(plan->log_rate, plan->passes, plan->starts, ut);
	if (rc != BN_OK) return rc;
	if (!plan->ut_dev)
		if ((rc = dev_alloc(&plan->ut_dev, ut.size() * sizeof(uint32_t))) != BN_OK) return rc;
	BN_HIP(hipMemcpy(plan->ut_dev, ut.data(), ut.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
	int cus = 0;
	BN_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, plan->device));
	plan->num_cus = std::max(cus, 1);
	return BN_OK;
}

// the device side of a new plan: the subspace table, and the pass tables where the fast path applies
static int plan_to_device(bn_antt_plan* p) {
	BN_DEVICE_SCOPE(p->device);
	if (int rc = dev_alloc(&p->s_dev, std::max<size_t>(p->s_host.size(), 1) * sizeof(uint32_t))) return rc;
	if (!p->s_host.empty()) BN_HIP(hipMemcpy(p->s_dev, p->s_host.data(), p->s_host.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
	if (bs_supports(p->log_h, p->log_rate)) {
		if (int rc = bs_prepare(p)) return rc;
		p->variant = bs_dev_knobs().variant;  // 5 (mixed register and LDS tiles) outside the development build
	}
	return BN_OK;
}

}  // namespace bn

using namespace bn;

extern "C" int bn_antt_plan_create(int device, int field_bits, int log_h, int log_rate, bn_antt_plan** out) {
	BN_CHECK_ARG(out != nullptr, "plan output pointer is NULL");
	*out = nullptr;
	BN_CHECK_ARG(field_bits == 32 || field_bits == 128, "field_bits must be 32 or 128 (got %d)", field_bits);
	BN_CHECK_ARG(log_h >= 1, "log_h must be >= 1 (got %d)", log_h);
	BN_CHECK_ARG(log_rate >= 0 && log_rate <= 4, "log_rate must be in [0,4] (got %d)", log_rate);
	BN_CHECK_ARG(log_h + log_rate <= field_bits, "log_h + log_rate must be <= %d", field_bits);
	if (log_h + log_rate > 32)
		BN_FAIL(BN_ERR_UNSUPPORTED, "log_h + log_rate > 32 is not built (every twiddle must lie in GF(2^32))");
	int ndev = 0;
	BN_HIP(hipGetDeviceCount(&ndev));
	BN_CHECK_ARG(device >= 0 && device < ndev, "device %d out of range (%d visible)", device, ndev);
	bn_antt_plan* p = new bn_antt_plan();
	p->device = device;
	p->field_bits = field_bits;
	p->log_h = log_h;
	p->log_rate = log_rate;
	p->limbs = field_bits / 32;
	p->width = log_h + log_rate - 1;
	subspace_evals(log_h, log_rate, p->s_host);
	p->variant = 0;
	if (const int rc = plan_to_device(p)) {
		bn_antt_plan_destroy(p);
		return rc;
	}
	*out = p;
	return BN_OK;
}

extern "C" int bn_antt_plan_destroy(bn_antt_plan* p) {
	if (!p) return BN_OK;
	DeviceScope ds(p->device);
	if (p->s_dev) (void)hipFree(p->s_dev);
	if (p->ut_dev) (void)hipFree(p->ut_dev);
	if (p->h_dev_in) (void)hipFree(p->h_dev_in);
	if (p->h_dev_out) (void)hipFree(p->h_dev_out);
	for (const auto& q : p->pending) {
		(void)hipEventSynchronize(q.end);
		(void)hipEventDestroy(q.begin);
		(void)hipEventDestroy(q.end);
	}
	for (auto e : p->ev_pool) (void)hipEventDestroy(e);
	if (p->own_stream) (void)hipStreamDestroy(p->own_stream);
	delete p;
	return BN_OK;
}

static int forward_device_impl(bn_antt_plan* p, const void* d_in, void* d_out, size_t batch, hipStream_t st) {
	const size_t n_in = ((size_t)1 << p->log_h) * p->limbs;
	const size_t n_out = n_in << p->log_rate;
	if (p->variant != 0) return launch_bs(p, (const uint32_t*)d_in, (uint32_t*)d_out, batch, st);
	for (size_t b = 0; b < batch; b++) {
		int rc = launch_v0(p, (const uint32_t*)d_in + b * n_in, (uint32_t*)d_out + b * n_out, false, 0, st);
		if (rc != BN_OK) return rc;
	}
	return BN_OK;
}

static int inverse_device_impl(bn_antt_plan* p, const void* d_in, void* d_out, int coset, size_t batch, hipStream_t st) {
	if (p->variant != 0) return launch_inv_bs(p, (const uint32_t*)d_in, (uint32_t*)d_out, coset, batch, st);
	const size_t n_words = ((size_t)1 << p->log_h) * p->limbs;
	for (size_t b = 0; b < batch; b++) {
		int rc = launch_v0(p, (const uint32_t*)d_in + b * n_words, (uint32_t*)d_out + b * n_words, true, coset, st);
		if (rc != BN_OK) return rc;
	}
	return BN_OK;
}

// bytes of `batch` blocks of 2^log_h elements
static size_t block_bytes(const bn_antt_plan* p, size_t batch) { return ((size_t)1 << p->log_h) * p->limbs * 4 * batch; }

extern "C" int bn_antt_forward_device(bn_antt_plan* p, const void* d_in, void* d_out, size_t batch, void* stream) {
	if (int rc = check_device_args(p, d_in, d_out, batch)) return rc;
	BN_CHECK_IO_DISJOINT(d_in, block_bytes(p, batch), d_out, block_bytes(p, batch) << p->log_rate);
	BN_DEVICE_SCOPE(p->device);
	return forward_device_impl(p, d_in, d_out, batch, (hipStream_t)stream);
}

extern "C" int bn_antt_inverse_device(bn_antt_plan* p, const void* d_in, void* d_out, int coset, size_t batch,
                                      void* stream) {
	if (int rc = check_device_args(p, d_in, d_out, batch)) return rc;
	BN_CHECK_ARG(coset >= 0 && coset < (1 << p->log_rate), "coset must be in [0, 2^%d) (got %d)", p->log_rate, coset);
	BN_CHECK_IO_DISJOINT(d_in, block_bytes(p, batch), d_out, block_bytes(p, batch));
	BN_DEVICE_SCOPE(p->device);
	return inverse_device_impl(p, d_in, d_out, coset, batch, (hipStream_t)stream);
}

static int check_host_args(const bn_antt_plan* p, const void* in, size_t in_elems, const void* out) {
	BN_CHECK_ARG(p != nullptr, "plan is NULL");
	BN_CHECK_ARG(in != nullptr && out != nullptr, "host buffers must be non-NULL");
	BN_CHECK_ARG(in_elems == ((size_t)1 << p->log_h), "input has %zu elements, plan expects 2^%d", in_elems, p->log_h);
	return BN_OK;
}
// Host in -> host out, synchronous, one transform: a staged call through the plan's staging buffers
// (allocated on first use: 2^log_h elements in, every coset block out, which holds the inverse's one
// block too) and its own stream. `launch(d_in, d_out, stream)` runs the transform between the copies.
template <class Launch>
static int host_transform(bn_antt_plan* p, const void* in, void* out, size_t out_bytes, Launch launch) {
	BN_DEVICE_SCOPE(p->device);
	const size_t in_bytes = block_bytes(p, 1);
	if (!p->h_dev_in)
		if (int rc = dev_alloc(&p->h_dev_in, in_bytes)) return rc;
	if (!p->h_dev_out)
		if (int rc = dev_alloc(&p->h_dev_out, in_bytes << p->log_rate)) return rc;
	if (!p->own_stream) BN_HIP(hipStreamCreateWithFlags(&p->own_stream, hipStreamNonBlocking));
	return staged_call(p->own_stream, in, p->h_dev_in, in_bytes, p->h_dev_out, out, out_bytes,
	                   [&](hipStream_t st) { return launch(p->h_dev_in, p->h_dev_out, st); });
}

// AdditiveNTT::apply (additive_ntt.cuh:201-265)
extern "C" int bn_antt_forward_host(bn_antt_plan* p, const void* in, size_t in_elems, void* out) {
	if (int rc = check_host_args(p, in, in_elems, out)) return rc;
	return host_transform(p, in, out, block_bytes(p, 1) << p->log_rate,
	                      [&](const void* d_in, void* d_out, hipStream_t st) { return forward_device_impl(p, d_in, d_out, 1, st); });
}

extern "C" int bn_antt_inverse_host(bn_antt_plan* p, const void* in, size_t in_elems, int coset, void* out) {
	if (int rc = check_host_args(p, in, in_elems, out)) return rc;
	BN_CHECK_ARG(coset >= 0 && coset < (1 << p->log_rate), "coset must be in [0, 2^%d) (got %d)", p->log_rate, coset);
	return host_transform(p, in, out, block_bytes(p, 1), [&](const void* d_in, void* d_out, hipStream_t st) {
		return inverse_device_impl(p, d_in, d_out, coset, 1, st);
	});
}

extern "C" int bn_antt_get_subspace_evals(const bn_antt_plan* p, uint32_t* out, size_t out_words) {
	BN_CHECK_ARG(p != nullptr && out != nullptr, "NULL argument");
	BN_CHECK_ARG(out_words >= (size_t)p->log_h * (size_t)p->width, "output too small");
	memcpy(out, p->s_host.data(), (size_t)p->log_h * (size_t)p->width * sizeof(uint32_t));
	return BN_OK;
}

extern "C" int bn_antt_plan_query(const bn_antt_plan* p, int what, int64_t* value) {
	BN_CHECK_ARG(p != nullptr && value != nullptr, "NULL argument");
	switch (what) {
		case 0: *value = p->log_h; break;
		case 1: *value = p->log_rate; break;
		case 2: *value = p->field_bits; break;
		case 3: *value = p->device; break;
		case 4: *value = p->variant; break;
		default: BN_FAIL(BN_ERR_INVALID, "unknown query %d", what);
	}
	return BN_OK;
}

extern "C" int bn_antt_plan_set_variant(bn_antt_plan* p, int variant) {
	BN_CHECK_ARG(p != nullptr, "plan is NULL");
	BN_CHECK_ARG(valid_variant(variant), "variant must be 0, 1, 4 or 5 (got %d)", variant);
	if (variant != 0 && !bs_supports(p->log_h, p->log_rate)) BN_FAIL(BN_ERR_UNSUPPORTED, "variants 1, 4 and 5 need log_h >= 12");
	if (variant != 0 && p->variant == 0) {
		BN_DEVICE_SCOPE(p->device);
		if (int rc = bs_prepare(p)) return rc;
	}
	p->variant = variant;
	return BN_OK;
}

extern "C" int bn_antt_set_event_timing(bn_antt_plan* p, int enable) {
	BN_CHECK_ARG(p != nullptr, "plan is NULL");
	int rc = timing_resolve(p);  // drop what an earlier timing window left
	if (rc != BN_OK) return rc;
	p->timing = enable;
	p->kind_ms.clear();
	p->kind_cnt.clear();
	return BN_OK;
}

extern "C" int bn_antt_time_passes(bn_antt_plan* p, const void* d_in, void* d_out, size_t batch, int reps,
                                   void* stream, float* ms_per_pass, int max_passes, int* n_passes) {
	BN_CHECK_ARG(p != nullptr && d_in != nullptr && d_out != nullptr && ms_per_pass != nullptr && n_passes != nullptr,
	             "NULL argument");
	BN_CHECK_ARG(batch >= 1 && reps >= 1, "batch and reps must be >= 1");
	if (p->variant == 0) BN_FAIL(BN_ERR_UNSUPPORTED, "pass timing is built for kernel variants 1, 4 and 5");
	BN_DEVICE_SCOPE(p->device);
	return bs_time_passes(p, (const uint32_t*)d_in, (uint32_t*)d_out, batch, reps, (hipStream_t)stream, ms_per_pass, max_passes,
	                      n_passes);
}

extern "C" int bn_antt_pass_kernel_name(bn_antt_plan* p, int pass, char* buf, size_t cap) {
	BN_CHECK_ARG(p != nullptr && buf != nullptr && cap > 0, "NULL argument");
	const void* fn = p->variant != 0 ? bs_pass_kernel(p, pass) : nullptr;
	if (!fn) BN_FAIL(BN_ERR_UNSUPPORTED, "no kernel name for pass %d of variant %d", pass, p->variant);
	const char* mangled = hipKernelNameRefByPtr(fn, nullptr);
	if (!mangled) BN_FAIL(BN_ERR_HIP, "hipKernelNameRefByPtr failed");
	int st = 0;
	char* dem = abi::__cxa_demangle(mangled, nullptr, nullptr, &st);
	snprintf(buf, cap, "%s", (st == 0 && dem) ? dem : mangled);
	free(dem);
	return BN_OK;
}

extern "C" int bn_antt_get_event_timing(bn_antt_plan* p, float* ms, int max_kinds, int* n_kinds) {
	BN_CHECK_ARG(p != nullptr && n_kinds != nullptr, "NULL argument");
	int rc = timing_resolve(p);
	if (rc != BN_OK) return rc;
	*n_kinds = (int)p->kind_ms.size();
	for (int i = 0; i < *n_kinds && i < max_kinds; i++) ms[i] = p->kind_cnt[i] ? p->kind_ms[i] / p->kind_cnt[i] : 0.f;
	return BN_OK;
}
