// The GF(2^128) sumcheck prover's state and the launch entry points of sumcheck.hip, shared with the
// prover's life cycle and round state machine (sc_prover.cpp). Internal to the library.
#pragma once

#include <stdlib.h>

#include "common.hpp"
#include "sc_rounds.hpp"

struct bn_sumcheck {
	int device = 0;
	int num_vars = 0, d = 0;
	int rank = 0, world = 1;
	int round = 0;
	size_t cur = 0;         // evaluations per column held by this prover
	size_t col_words = 0;   // words between columns (allocation)
	uint32_t* cols = nullptr;
	uint32_t* acc = nullptr;    // 2 sets of kAccSet words (see kAccCopies), alternating rounds
	int par = 0;                // set used by the next round_messages
	uint32_t* h_res = nullptr;  // host-mapped, GPU-coherent: the round's points + sequence word
	uint32_t* sink = nullptr;   // caller's device buffer for the raw point words (sharded exchange)
	uint32_t* d_res = nullptr;  // its device address
	uint32_t seq = 0;
	hipStream_t stream = nullptr;
	bool sharded_used = false;
	// bn_sumcheck_create_staged leaves compact input untransposed until bn_sumcheck_prepare (the
	// reference constructor's separate Memcpy and Transpose phases, sumcheck.cuh:88-124)
	bool prepared = true;
	int compact_input = 0;
	// Round claim: once round i's points are known, move_to_next_round(r) interpolates them at r,
	// which is this prover's sum for round i + 1 (p_i(r) = sum_x prod_j f_j'(x), per shard too).
	// Round i + 1 then skips point 1 (p(1) = claim + p(0)): (d - 1) fewer products per pair.
	// The interpolation itself runs in the next round_messages, while its kernel is in flight.
	bool have_pts = false, have_claim = false, claim_pending = false;
	// bn_sumcheck_round_messages_sink: the round's points went to the sink unread by the prover; the
	// caller (the sharded driver) holds the GLOBAL points and completes a skipped p(1) itself
	bool pts_external = false;
	// the round read last: what a repeated round_messages returns and, while have_pts, what the
	// next claim is interpolated from (the final evaluation, cur == 1, leaves have_pts false)
	uint32_t last_sum[4] = {0, 0, 0, 0}, last_points[4 * (bn::quad::kMaxD + 1)];
	uint32_t claim[4], pending_r[4];
	// move_to_next_round queues the next round's messages kernel right behind the fold, so the
	// GPU never waits for the host's next call (composition_eval, which only folds, does not)
	bool msgs_queued = false, eager = true;
	// BN_SUMCHECK_FULL_POINTS=1 (read when the prover is created): every round computes p(1) and
	// the sum from the data instead of deriving them from the claim, so the verifier's
	// p(0) + p(1) == previous p(r) check also tests the folds (tests/test_gpu_sumcheck.py)
	bool derive_p1 = !(getenv("BN_SUMCHECK_FULL_POINTS") && atoi(getenv("BN_SUMCHECK_FULL_POINTS")) != 0);
	bn::ScKnobs knobs = bn::sc_dev_knobs();
	// round server (sc_server) for the last rounds: running once launched until cur == 1
	struct {
		uint32_t* h_ctl = nullptr;  // host-mapped control words (challenge, skip flag, ticket)
		bool running = false;
		uint32_t ticket = 0;
		unsigned long long* h_trace = nullptr;  // knobs.timing: the server's phase stamps
		double t_post = 0;                      // ... and the host's time of the last challenge post
	} srv;
	bool read_this_round = false;
	bool gathered = false;  // built by bn_sumcheck_import_gathered (no round server: server_eligible)
};

namespace bn {

// a shard is down to one batch: its rounds continue on the gathered replica
inline bool shard_exhausted(const bn_sumcheck* sc) { return sc->world > 1 && sc->cur <= 32; }

// The round server takes over once at most knobs.server_max_cur evaluations per column are left: an
// unsharded, eager prover without a message sink (composition_eval only folds). Not a replica built
// by import_gathered: the sharded driver runs one per rank in lockstep, and several servers
// waiting in one process would block each other's queues for up to the timeout.
inline bool server_eligible(const bn_sumcheck* sc) {
	return sc->eager && sc->world == 1 && !sc->sink && !sc->gathered && sc->prepared && sc->cur >= 2 &&
	       sc->cur <= sc->knobs.server_max_cur;
}

// sumcheck.hip
int sc_kernels_init(bn_sumcheck* sc);  // raises the dynamic-LDS limit of every kernel
int sc_launch(bn_sumcheck* sc, bool fold, const uint32_t* r);
// a server that folds `cur` evaluations per column on `ticket` and posts those messages as `seq`
int server_launch(bn_sumcheck* sc, size_t cur, uint32_t seq, uint32_t ticket);
// hand the server its next challenge (the fold of this round, then the next round's messages)
void server_post(bn_sumcheck* sc, const uint32_t* r, bool skip1);
void server_stop(bn_sumcheck* sc);       // release a server still waiting for a challenge
bool server_exited_at(const bn_sumcheck* sc, uint32_t ticket);  // it timed out after serving `ticket`
int wait_posted(bn_sumcheck* sc);

}  // namespace bn
