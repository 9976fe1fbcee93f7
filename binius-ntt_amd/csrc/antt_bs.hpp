// Host interface between the bitsliced additive-NTT kernel files (antt_bs.hip variant 1, antt_rr.hip
// variant 4; variant 5 = both; antt_inv.hip the inverse) and the plan management in antt.hip. The
// pass tables themselves are planned in antt_passes.cpp and held by the plan.
#pragma once

#include <stdint.h>

#include "antt_passes.hpp"
#include "antt_plan.hpp"

namespace bn {

// The environment switches of the development build (make BN_DEV=1), read once per call by
// dev_knobs() in antt_bs.hip; the product build leaves the defaults.
struct BsDevKnobs {
	int dbg = 0, split = -1, rr_last = -1;
	bool trace = false;
};

// "Fewer tiles than two per CU": such a launch runs at most one wave per SIMD whatever the kernel's
// register count, and picks the kernels built for that (use_split, use_rr_last, rr_pass_kernel).
inline bool small_launch(const bn_antt_plan* plan, size_t ntiles) { return ntiles < (size_t)2 * (size_t)plan->num_cus; }

// Bitsliced fast path, used when bs_supports(log_h, log_rate); bs_prepare sets the plan up for it
// (pass tables, kernel attributes) on creation and on the first change from variant 0.
int bs_prepare(bn_antt_plan* plan);
int launch_bs(bn_antt_plan* plan, const uint32_t* d_in, uint32_t* d_out, size_t batch, hipStream_t st);
int bs_time_passes(bn_antt_plan* plan, const uint32_t* d_in, uint32_t* d_out, size_t batch, int reps, hipStream_t st,
                   float* ms, int max_passes, int* n_out);
const void* bs_pass_kernel(bn_antt_plan* plan, int i);
// its inverse (antt_inv.hip): one coset block of evaluations back to coefficients
int launch_inv_bs(bn_antt_plan* plan, const uint32_t* d_in, uint32_t* d_out, int coset, size_t batch, hipStream_t st);
// variant 4 (antt_rr.hip): register-tile kernels over the same passes.
int rr_prepare(bn_antt_plan* plan);
// the register-tile kernel of a pass launched over `ntiles` tiles (select_pass asks, nobody else)
const void* rr_pass_kernel(const bn_antt_plan* plan, const BsPass& pass, size_t ntiles);
// pass i (timing kind) on `kernel`, as select_pass decided, with the plan's cached table of the pass
int rr_launch_pass(bn_antt_plan* plan, int i, const RtPass& rt, const void* kernel, size_t ntiles, const BsDevKnobs& kn,
                   const uint32_t* d_in, uint32_t* d_out, hipStream_t st);

}  // namespace bn
