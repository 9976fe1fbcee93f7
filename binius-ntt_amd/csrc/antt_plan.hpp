// Additive-NTT plan: host-side twiddle precomputation and launch bookkeeping.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "antt_passes.hpp"
#include "common.hpp"

struct bn_antt_plan {
	int device = 0;
	int field_bits = 128;
	int log_h = 0;
	int log_rate = 0;
	int limbs = 4;   // u32 words per element
	int width = 0;   // log_h + log_rate - 1 (columns of the subspace table)
	int variant = 0; // kernel path in use (see antt.hip)
	int num_cus = 0; // compute units of the device (launches below two tiles per CU pick other kernels)
	std::vector<uint32_t> s_host;  // log_h x width, row-major
	uint32_t* s_dev = nullptr;     // same on the device
	// pass tables of the bitsliced kernels and the register-tile table of every pass (antt_passes.cpp),
	// filled once by bs_prepare; empty for variant-0 plans
	std::vector<bn::BsPass> passes;
	std::vector<bn::RtPass> rt;
	// the tile start of every pass and, on the device, the chunk tables of all of them
	// (plan_tile_starts): written once by bs_prepare, read by every pass kernel, freed with the plan
	std::vector<bn::TileStart> starts;
	uint32_t* ut_dev = nullptr;
	hipStream_t own_stream = nullptr;
	// host-apply staging
	void* h_dev_in = nullptr;
	void* h_dev_out = nullptr;
	// optional per-launch event timing: events are recorded around each pass without any host
	// synchronisation (the passes stay back to back) and resolved by bn_antt_get_event_timing
	int timing = 0;
	struct PendingPass {
		int kind;
		hipEvent_t begin, end;
	};
	std::vector<hipEvent_t> ev_pool;
	std::vector<PendingPass> pending;
	hipEvent_t cur_begin = nullptr;
	std::vector<float> kind_ms;
	std::vector<int> kind_cnt;
};

namespace bn {
// The argument checks of every *_device entry point (forward, inverse, fold): the plan, the buffers
// and the batch; each call then adds its own checks and BN_CHECK_IO_DISJOINT.
inline int check_device_args(const bn_antt_plan* p, const void* d_in, const void* d_out, size_t batch) {
	BN_CHECK_ARG(p != nullptr, "plan is NULL");
	BN_CHECK_ARG(d_in != nullptr && d_out != nullptr, "device buffers must be non-NULL");
	BN_CHECK_ARG(batch >= 1, "batch must be >= 1");
	return BN_OK;
}
// hipEvent timing around one launch of pass `kind` (no-op unless plan->timing).
int timing_begin(bn_antt_plan* p, int kind, hipStream_t st);
int timing_end(bn_antt_plan* p, int kind, hipStream_t st);
}  // namespace bn
