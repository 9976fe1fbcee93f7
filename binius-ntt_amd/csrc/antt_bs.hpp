// Host interface between the bitsliced additive-NTT kernel files (antt_bs.hip variant 1, antt_rr.hip
// variant 4; variant 5 = both; antt_inv.hip the inverse) and the plan management in antt.hip. The
// pass tables and the kernel of every launch are planned in antt_passes.cpp.
#pragma once

#include <stdint.h>

#include <utility>

#include "antt_passes.hpp"
#include "antt_plan.hpp"

namespace bn {

// What runs `pass` of `batch` transforms: ntt_plan_launch on the plan's facts (the inverse reads and
// writes one coset block per transform). Every launch and bs_pass_kernel go through here.
inline NttLaunch plan_pass(const bn_antt_plan* plan, const BsPass& pass, bool inverse, size_t batch, const BsDevKnobs& kn) {
	const size_t ntiles = (batch << (inverse ? 0 : plan->log_rate)) << pass.n_outer;
	return ntt_plan_launch(plan->limbs, plan->variant, inverse, pass.role, pass_fmax(pass), ntiles, plan->num_cus, kn);
}

// Entry `instance` of kNttInstances as a kernel (antt.hip asks the file of its family); each file
// instantiates its families' entries of the list through instance_table (common.hpp)
const void* ntt_kernel_fn(int instance);
const void* bs_kernel_fn(int instance);   // antt_bs.hip: antt_bs_pass, antt_bs3_pass
const void* rr_kernel_fn(int instance);   // antt_rr.hip: antt_rr_pass
const void* inv_kernel_fn(int instance);  // antt_inv.hip: antt_inv_bs_pass

// Bitsliced fast path, used when bs_supports(log_h, log_rate)
int launch_bs(bn_antt_plan* plan, const uint32_t* d_in, uint32_t* d_out, size_t batch, hipStream_t st);
int bs_time_passes(bn_antt_plan* plan, const uint32_t* d_in, uint32_t* d_out, size_t batch, int reps, hipStream_t st,
                   float* ms, int max_passes, int* n_out);
const void* bs_pass_kernel(bn_antt_plan* plan, int i);
// its inverse (antt_inv.hip): one coset block of evaluations back to coefficients
int launch_inv_bs(bn_antt_plan* plan, const uint32_t* d_in, uint32_t* d_out, int coset, size_t batch, hipStream_t st);
// BN_TRACE (development build, antt_bs.hip): the zeroed per-wave stamp buffer of a launch, and its
// print-out as cycles per wave-tile
constexpr int kTraceSlots = 10;
int trace_buffer(size_t waves, hipStream_t st, unsigned long long** out);
int print_trace(int i, const NttLaunch& nl, int fmax, const unsigned long long* d_trace, size_t waves, hipStream_t st);
// pass i (timing kind) on register tiles (antt_rr.hip), as plan_pass decided
int rr_launch_pass(bn_antt_plan* plan, int i, const NttLaunch& nl, const BsDevKnobs& kn, const uint32_t* d_in, uint32_t* d_out,
                   hipStream_t st);

}  // namespace bn
