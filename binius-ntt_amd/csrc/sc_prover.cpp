// GF(2^128) sumcheck prover: life cycle, sharding and the round state machine behind the C ABI,
// and the verifier's composition evaluation. The kernels and their launches are in sumcheck.hip.
#include "sc_prover.hpp"

#include <string.h>

#include <atomic>
#include <memory>
#include <vector>

int bitslice_launch(const void* src, void* dst, size_t nblk, int untranspose, hipStream_t st);  // field.hip

namespace {

using namespace bn;
using namespace bn::quad;

void sc_free(bn_sumcheck* sc) {
	if (!sc) return;
	server_stop(sc);
	if (sc->stream) (void)hipStreamSynchronize(sc->stream);
	if (sc->cols) (void)hipFree(sc->cols);
	if (sc->acc) (void)hipFree(sc->acc);
	if (sc->h_res) (void)hipHostFree(sc->h_res);
	if (sc->srv.h_ctl) (void)hipHostFree(sc->srv.h_ctl);
	if (sc->srv.h_trace) (void)hipHostFree(sc->srv.h_trace);
	if (sc->stream) (void)hipStreamDestroy(sc->stream);
	delete sc;
}

// A prover under construction: freed on every way out of its constructor but release()
struct ScFree {
	void operator()(bn_sumcheck* sc) const { sc_free(sc); }
};
using ScOwner = std::unique_ptr<bn_sumcheck, ScFree>;

int check_shape(int num_vars, int d, int transposed) {
	BN_CHECK_ARG(d >= 1 && d <= kMaxD, "composition_size must be in [1, %d]", kMaxD);
	BN_CHECK_ARG(num_vars >= 1 && num_vars <= 30, "num_vars must be in [1, 30]");
	BN_CHECK_ARG(!transposed || num_vars >= 5, "bitsliced input needs num_vars >= 5 (whole 32-element batches)");
	return BN_OK;
}

int check_shard(int num_vars, int rank, int world) {
	BN_CHECK_ARG(world >= 1 && (world & (world - 1)) == 0, "world must be a power of two");
	BN_CHECK_ARG(rank >= 0 && rank < world, "rank out of range");
	BN_CHECK_ARG(((size_t)1 << num_vars) >= (size_t)32 * world, "need at least one 32-element batch per rank");
	return BN_OK;
}

// A new prover on the current device: its stream, accumulator sets, host-mapped result and control
// words, and (col_words != 0) its own column storage.
int sc_new(int device, int num_vars, int d, size_t col_words, ScOwner& out) {
	ScOwner sc(new bn_sumcheck);
	sc->device = device;
	sc->num_vars = num_vars;
	sc->d = d;
	BN_HIP(hipStreamCreateWithFlags(&sc->stream, hipStreamNonBlocking));
	if (const int rc = dev_alloc(&sc->acc, sizeof(uint32_t) * 2 * kAccSet)) return rc;
	BN_HIP(hipMemsetAsync(sc->acc, 0, sizeof(uint32_t) * 2 * kAccSet, sc->stream));
	BN_HIP(hipHostMalloc((void**)&sc->h_res, sizeof(uint32_t) * (kResSeq + 1), hipHostMallocMapped | hipHostMallocCoherent));
	memset(sc->h_res, 0, sizeof(uint32_t) * (kResSeq + 1));
	BN_HIP(hipHostGetDevicePointer((void**)&sc->d_res, sc->h_res, 0));
	if (const int rc = sc_kernels_init(sc.get())) return rc;
	if (col_words) {
		sc->col_words = col_words;
		if (const int rc = dev_alloc(&sc->cols, sizeof(uint32_t) * col_words * (size_t)d)) return rc;
	}
	out = std::move(sc);
	return BN_OK;
}

// order the prover's stream after the work already queued on `other`
int order_after(bn_sumcheck* sc, hipStream_t other) {
	hipEvent_t ready = nullptr;
	hipError_t e = hipEventCreateWithFlags(&ready, hipEventDisableTiming);
	if (e == hipSuccess) e = hipEventRecord(ready, other);
	if (e == hipSuccess) e = hipStreamWaitEvent(sc->stream, ready, 0);
	if (ready) (void)hipEventDestroy(ready);
	if (e != hipSuccess) BN_FAIL(BN_ERR_HIP, "ordering the prover's stream after the producer's: %s", hipGetErrorString(e));
	return BN_OK;
}

// d columns of in_words words at `src` into the prover's (zero-padded) column storage
int copy_columns(bn_sumcheck* sc, const uint32_t* src, size_t in_words, hipMemcpyKind kind) {
	if (sc->col_words != in_words) BN_HIP(hipMemsetAsync(sc->cols, 0, sizeof(uint32_t) * sc->col_words * (size_t)sc->d, sc->stream));
	for (int j = 0; j < sc->d; j++)
		BN_HIP(hipMemcpyAsync(sc->cols + (size_t)j * sc->col_words, src + (size_t)j * in_words, sizeof(uint32_t) * in_words, kind,
		                      sc->stream));
	return BN_OK;
}

// Device bit-transpose of compact input (the reference constructor's transpose_kernel,
// sumcheck.cuh:97-101), then a stream synchronisation: the prover is ready for round 0.
int sc_prepare(bn_sumcheck* sc) {
	if (sc->prepared) return BN_OK;
	if (sc->compact_input) {
		const size_t blocks = sc->col_words / 128 * (size_t)sc->d;
		if (const int rc = bn_bitslice_device(sc->cols, blocks, 0, sc->stream)) return rc;
	}
	BN_HIP(hipStreamSynchronize(sc->stream));
	sc->prepared = true;
	return BN_OK;
}

// Common tail of the constructors from whole columns: the d columns (4*2^n words each, compact or
// bitsliced) are in the prover's storage; compact ones are converted in place unless `stage_only`.
int sc_finish_create(bn_sumcheck* sc, int transposed, bool stage_only = false) {
	sc->compact_input = !transposed;
	sc->prepared = false;
	sc->cur = (size_t)1 << sc->num_vars;
	sc->round = 0;
	if (!stage_only) return sc_prepare(sc);
	BN_HIP(hipStreamSynchronize(sc->stream));
	return BN_OK;
}

int queue_messages(bn_sumcheck* sc) {
	if (const int rc = sc_launch(sc, false, nullptr)) return rc;
	sc->par ^= 1;
	sc->msgs_queued = true;
	return BN_OK;
}

int create_from_host(int device, int num_vars, int d, int transposed, const uint32_t* evals, bool stage_only, bn_sumcheck** out) {
	BN_CHECK_ARG(out, "NULL output pointer");
	*out = nullptr;
	BN_CHECK_ARG(evals, "NULL evals");
	int rc = check_shape(num_vars, d, transposed);
	if (rc != BN_OK) return rc;
	BN_DEVICE_SCOPE(device);
	const size_t in_words = (size_t)4 << num_vars;
	ScOwner sc;
	if ((rc = sc_new(device, num_vars, d, in_words < 128 ? 128 : in_words, sc)) != BN_OK) return rc;  // pad to one batch
	if ((rc = copy_columns(sc.get(), evals, in_words, hipMemcpyHostToDevice)) != BN_OK) return rc;
	if ((rc = sc_finish_create(sc.get(), transposed, stage_only)) != BN_OK) return rc;
	*out = sc.release();
	return BN_OK;
}

}  // namespace

extern "C" int bn_sumcheck_create(int device, int num_vars, int d, int transposed, const uint32_t* evals, bn_sumcheck** out) {
	return create_from_host(device, num_vars, d, transposed, evals, false, out);
}

extern "C" int bn_sumcheck_create_staged(int device, int num_vars, int d, int transposed, const uint32_t* evals, bn_sumcheck** out) {
	return create_from_host(device, num_vars, d, transposed, evals, true, out);
}

extern "C" int bn_sumcheck_prepare(bn_sumcheck* sc) {
	BN_CHECK_ARG(sc, "NULL prover");
	BN_DEVICE_SCOPE(sc->device);
	return sc_prepare(sc);
}

extern "C" int bn_sumcheck_create_device(int device, int num_vars, int d, int transposed, void* d_evals, int take, bn_sumcheck** out) {
	BN_CHECK_ARG(out, "NULL output pointer");
	*out = nullptr;
	BN_CHECK_ARG(d_evals, "NULL evals");
	int rc = check_shape(num_vars, d, transposed);
	if (rc != BN_OK) return rc;
	BN_DEVICE_SCOPE(device);
	const size_t in_words = (size_t)4 << num_vars;
	const bool adopt = take && in_words >= 128;  // the caller's buffer becomes the column storage
	ScOwner sc;
	if ((rc = sc_new(device, num_vars, d, adopt ? 0 : in_words < 128 ? 128 : in_words, sc)) != BN_OK) return rc;
	// after the work already queued on the legacy default stream (producers on other streams must
	// still complete first: see the header)
	if ((rc = order_after(sc.get(), nullptr)) != BN_OK) return rc;
	if (adopt) {
		sc->cols = (uint32_t*)d_evals;
		sc->col_words = in_words;
	} else {
		if (!transposed && sc->col_words == in_words) {
			// compact columns of whole blocks: bit-transposed straight from the caller's buffer into the
			// prover's storage (one pass over HBM instead of a copy and an in-place transpose)
			if ((rc = bitslice_launch(d_evals, sc->cols, in_words / 128 * (size_t)d, 0, sc->stream)) != BN_OK) return rc;
			transposed = 1;
		} else if ((rc = copy_columns(sc.get(), (const uint32_t*)d_evals, in_words, hipMemcpyDeviceToDevice)) != BN_OK) {
			return rc;
		}
		if (take) {
			BN_HIP(hipStreamSynchronize(sc->stream));
			BN_HIP(hipFree(d_evals));
		}
	}
	if ((rc = sc_finish_create(sc.get(), transposed)) != BN_OK) return rc;
	*out = sc.release();
	return BN_OK;
}

// A shard prover built straight from this rank's share of bitsliced columns (the batches b with
// b mod world == rank, in order: 4 * 2^num_vars / world words per column, columns back to back),
// so no rank ever holds the whole input. The copy is ordered after the work queued on `stream`
// (the caller's producer stream; NULL = the legacy default stream).
extern "C" int bn_sumcheck_create_shard_device(int device, int num_vars, int d, int rank, int world, const void* d_local, void* stream,
                                               bn_sumcheck** out) {
	BN_CHECK_ARG(out, "NULL output pointer");
	*out = nullptr;
	BN_CHECK_ARG(d_local, "NULL evals");
	int rc = check_shape(num_vars, d, 1);
	if (rc != BN_OK || (rc = check_shard(num_vars, rank, world)) != BN_OK) return rc;
	BN_DEVICE_SCOPE(device);
	const size_t n = (size_t)1 << num_vars;
	ScOwner sc;
	if ((rc = sc_new(device, num_vars, d, 4 * n / (size_t)world, sc)) != BN_OK) return rc;
	if ((rc = order_after(sc.get(), (hipStream_t)stream)) != BN_OK) return rc;
	BN_HIP(hipMemcpyAsync(sc->cols, d_local, sizeof(uint32_t) * sc->col_words * (size_t)d, hipMemcpyDeviceToDevice, sc->stream));
	BN_HIP(hipStreamSynchronize(sc->stream));
	sc->cur = n / (size_t)world;
	sc->round = 0;
	sc->rank = rank;
	sc->world = world;
	sc->sharded_used = world > 1;
	*out = sc.release();
	return BN_OK;
}

extern "C" int bn_sumcheck_set_shard(bn_sumcheck* sc, int rank, int world) {
	BN_CHECK_ARG(sc, "NULL prover");
	BN_CHECK_ARG(sc->round == 0 && !sc->sharded_used, "set_shard must precede the first round");
	int rc = check_shard(sc->num_vars, rank, world);
	if (rc != BN_OK) return rc;
	if (world == 1) return BN_OK;
	BN_DEVICE_SCOPE(sc->device);
	if ((rc = sc_prepare(sc)) != BN_OK) return rc;  // a staged prover transposes on first use
	// keep the batches b with b mod world == rank, in order
	const size_t n = (size_t)1 << sc->num_vars;
	const size_t nb_local = n / 32 / world;
	DevBuf local;  // freed unless released into the prover
	if ((rc = local.alloc(sizeof(uint32_t) * 128 * nb_local * (size_t)sc->d)) != BN_OK) return rc;
	uint32_t* const p = (uint32_t*)local.p;
	for (int j = 0; j < sc->d; j++)
		BN_HIP(hipMemcpy2DAsync(p + (size_t)j * 128 * nb_local, 128 * sizeof(uint32_t),
		                        sc->cols + (size_t)j * sc->col_words + 128 * (size_t)rank, 128 * sizeof(uint32_t) * world,
		                        128 * sizeof(uint32_t), nb_local, hipMemcpyDeviceToDevice, sc->stream));
	BN_HIP(hipStreamSynchronize(sc->stream));
	BN_HIP(hipFree(sc->cols));
	sc->cols = (uint32_t*)local.release();
	sc->col_words = 128 * nb_local;
	sc->cur = n / world;
	sc->rank = rank;
	sc->world = world;
	sc->sharded_used = true;
	return BN_OK;
}

extern "C" int bn_sumcheck_needs_gather(const bn_sumcheck* sc, int* flag) {
	BN_CHECK_ARG(sc && flag, "NULL argument");
	*flag = shard_exhausted(sc) ? 1 : 0;
	return BN_OK;
}

extern "C" int bn_sumcheck_export_shard(const bn_sumcheck* sc, uint32_t* out, size_t out_words) {
	BN_CHECK_ARG(sc && out, "NULL argument");
	BN_CHECK_ARG(shard_exhausted(sc), "export_shard is only valid once a shard is down to one batch");
	BN_CHECK_ARG(out_words >= (size_t)128 * sc->d, "output needs composition_size * 128 words");
	BN_DEVICE_SCOPE(sc->device);
	for (int j = 0; j < sc->d; j++)
		BN_HIP(hipMemcpyAsync(out + 128 * (size_t)j, sc->cols + (size_t)j * sc->col_words, 128 * sizeof(uint32_t), hipMemcpyDeviceToHost,
		                      sc->stream));
	BN_HIP(hipStreamSynchronize(sc->stream));
	return BN_OK;
}

extern "C" int bn_sumcheck_import_gathered(bn_sumcheck* sc, const uint32_t* words, size_t n_words, int world) {
	BN_CHECK_ARG(sc && words, "NULL argument");
	BN_CHECK_ARG(world == sc->world && shard_exhausted(sc), "import_gathered needs the exported state of every rank");
	BN_CHECK_ARG(n_words >= (size_t)world * 128 * sc->d, "need world * composition_size * 128 words");
	BN_DEVICE_SCOPE(sc->device);
	// rank r's batch becomes global batch r (r < world, so batch r is owned by rank r)
	const size_t col_words = 128 * (size_t)world;
	std::vector<uint32_t> host((size_t)sc->d * col_words);
	for (int r = 0; r < world; r++)
		for (int j = 0; j < sc->d; j++)
			memcpy(&host[(size_t)j * col_words + 128 * (size_t)r], words + ((size_t)r * sc->d + j) * 128, 128 * sizeof(uint32_t));
	DevBuf cols;  // freed unless released into the prover
	if (const int rc = cols.alloc(sizeof(uint32_t) * host.size())) return rc;
	BN_HIP(hipMemcpyAsync(cols.p, host.data(), sizeof(uint32_t) * host.size(), hipMemcpyHostToDevice, sc->stream));
	BN_HIP(hipStreamSynchronize(sc->stream));
	BN_HIP(hipFree(sc->cols));
	sc->cols = (uint32_t*)cols.release();
	sc->col_words = col_words;
	sc->cur = (size_t)32 * world;
	sc->rank = 0;
	sc->world = 1;
	sc->gathered = true;
	sc->have_pts = sc->have_claim = sc->claim_pending = sc->pts_external = false;  // the shards' claims are partial: recompute point 1
	sc->msgs_queued = false;
	return BN_OK;
}

extern "C" int bn_sumcheck_set_message_sink(bn_sumcheck* sc, void* d_words) {
	BN_CHECK_ARG(sc, "NULL prover");
	// a running round server posts to the host words only: switching the prover to a sink then would
	// hand the caller words no kernel wrote
	BN_CHECK_ARG(!sc->srv.running || d_words == sc->sink, "the round server is running: set the sink before the last rounds");
	sc->sink = (uint32_t*)d_words;
	return BN_OK;
}

extern "C" int bn_sumcheck_stream(const bn_sumcheck* sc, void** stream) {
	BN_CHECK_ARG(sc && stream, "NULL argument");
	*stream = (void*)sc->stream;
	return BN_OK;
}

extern "C" int bn_sumcheck_round_messages(bn_sumcheck* sc, uint32_t* sum, uint32_t* points) {
	BN_CHECK_ARG(sc && sum && points, "NULL argument");
	BN_CHECK_ARG(!shard_exhausted(sc), "shard exhausted: gather (export_shard/import_gathered) first");
	BN_DEVICE_SCOPE(sc->device);
	int rc = sc_prepare(sc);  // a staged prover transposes on first use
	if (rc != BN_OK) return rc;
	const int npts = sc->d + 1;
	if (!sc->msgs_queued && sc->srv.running) {
		// this round was read already and the server is waiting for the next challenge (no launch
		// may queue behind it): the same messages again
		if (!sc->read_this_round) BN_FAIL(BN_ERR_INVALID, "round server: no messages for this round");
		memcpy(sum, sc->last_sum, 16);
		memcpy(points, sc->last_points, sizeof(uint32_t) * 4 * npts);
		return BN_OK;
	}
	if (sc->claim_pending && sc->pts_external)  // checked before anything is queued
		BN_FAIL(BN_ERR_INVALID, "the previous round's points went to the message sink: read this round there too");
	if (!sc->msgs_queued && (rc = queue_messages(sc)) != BN_OK) return rc;
	sc->msgs_queued = false;
	if (sc->claim_pending) {  // last round's claim, computed while this round's kernel runs
		rc = bn_sumcheck_interpolate(sc->last_points, npts, sc->pending_r, sc->claim);
		if (rc != BN_OK) return rc;
		sc->claim_pending = false;
		sc->have_claim = sc->cur > 1;
	}
	if ((rc = wait_posted(sc)) != BN_OK) return rc;
	std::atomic_thread_fence(std::memory_order_acquire);
	uint32_t acc[4 * (kMaxD + 1)];
	for (int i = 0; i < 4 * npts; i++) acc[i] = ((const volatile uint32_t*)sc->h_res)[i];
	if (sc->cur == 1) {
		memcpy(sum, acc, 16);  // mode 2 computed prod_j f_j(0) as "point 0"
		memset(points, 0, sizeof(uint32_t) * 4 * npts);
		sc->have_pts = false;  // (last_points feeds no claim: nothing is left to fold)
	} else {
		memcpy(points, acc, sizeof(uint32_t) * 4 * npts);
		if (sc->have_claim) {
			// point 1 was skipped: p(1) = claim + p(0)
			for (int i = 0; i < 4; i++) points[4 + i] = sc->claim[i] ^ acc[i];
			memcpy(sum, sc->claim, 16);
		} else {
			for (int i = 0; i < 4; i++) sum[i] = acc[i] ^ acc[4 + i];
		}
		sc->have_pts = true;
		sc->pts_external = false;
	}
	sc->have_claim = false;
	sc->sharded_used = true;
	memcpy(sc->last_sum, sum, 16);
	memcpy(sc->last_points, points, sizeof(uint32_t) * 4 * npts);
	sc->read_this_round = true;
	return BN_OK;
}

extern "C" int bn_sumcheck_round_messages_sink(bn_sumcheck* sc) {
	BN_CHECK_ARG(sc, "NULL prover");
	BN_CHECK_ARG(sc->sink, "no message sink set (bn_sumcheck_set_message_sink)");
	BN_CHECK_ARG(!shard_exhausted(sc), "shard exhausted: gather (export_shard/import_gathered) first");
	BN_CHECK_ARG(!sc->srv.running, "the round server is running: read this round with bn_sumcheck_round_messages");
	BN_DEVICE_SCOPE(sc->device);
	int rc = sc_prepare(sc);
	if (rc != BN_OK) return rc;
	if (!sc->msgs_queued && (rc = queue_messages(sc)) != BN_OK) return rc;
	// no poll: the words reach the sink on the prover's stream, where the caller orders its reads.
	// The caller holds this round's global points, so the next round may skip p(1) (flag bit 0 of
	// sink word 36 says when it did)
	sc->msgs_queued = false;
	sc->claim_pending = sc->have_claim = false;
	sc->have_pts = sc->cur > 1;
	sc->pts_external = true;
	sc->sharded_used = true;
	return BN_OK;
}

extern "C" int bn_sumcheck_move_to_next_round(bn_sumcheck* sc, const uint32_t* challenge) {
	BN_CHECK_ARG(sc && challenge, "NULL argument");
	BN_CHECK_ARG(sc->cur >= 2, "no variables left to fold");
	BN_CHECK_ARG(!shard_exhausted(sc), "shard exhausted: gather (export_shard/import_gathered) first");
	BN_DEVICE_SCOPE(sc->device);
	int rc = sc_prepare(sc);  // a staged prover transposes on first use
	if (rc != BN_OK) return rc;
	const bool to_server = sc->srv.running || server_eligible(sc);
	// no sync: the fold is ordered before the next round's messages on the prover's stream
	sc->have_claim = false;  // a claim not consumed by this round's messages is stale now
	sc->claim_pending = sc->have_pts && sc->derive_p1;
	if (!to_server && (rc = sc_launch(sc, true, challenge)) != BN_OK) return rc;  // (a fold launch does not read the claim state)
	if (sc->claim_pending) memcpy(sc->pending_r, challenge, 16);
	sc->have_pts = false;
	sc->read_this_round = false;
	if (to_server) {
		// the round server folds and computes the next round's messages (p(1) skipped when the
		// claim is derived; never for the final evaluation, which the server decides itself)
		if (sc->srv.running && sc->msgs_queued) {
			// the previous challenge's messages were not read: let them land first (one ticket at a
			// time, so a relaunched server never misses an overwritten challenge)
			if ((rc = wait_posted(sc)) != BN_OK) return rc;
		}
		if (!sc->srv.running || server_exited_at(sc, sc->srv.ticket)) {
			if ((rc = server_launch(sc, sc->cur, sc->seq + 1, sc->srv.ticket + 1)) != BN_OK) return rc;
		}
		server_post(sc, challenge, sc->claim_pending && sc->cur / 2 >= 2);
	}
	sc->cur /= 2;
	sc->round++;
	sc->sharded_used = true;
	// the server's post is this round's queued messages; on the plain path a queued, unread messages
	// kernel ran before the fold and is dropped
	sc->msgs_queued = to_server;
	if (!to_server && sc->eager && !shard_exhausted(sc)) return queue_messages(sc);
	return BN_OK;
}

extern "C" int bn_sumcheck_round(const bn_sumcheck* sc, int* round) {
	BN_CHECK_ARG(sc && round, "NULL argument");
	*round = sc->round;
	return BN_OK;
}

extern "C" int bn_sumcheck_destroy(bn_sumcheck* sc) {
	if (!sc) return BN_OK;
	// (a failed switch must not leak the prover: free it on whichever device is current)
	DeviceScope ds(sc->device);
	sc_free(sc);
	return BN_OK;
}

// ---------------------------------------------------------------------------------------
// Verifier side
// ---------------------------------------------------------------------------------------

// Folding every column of the new prover `sc` at r_0, r_1, ... (highest variable first) leaves
// f_j(r); the last round's "sum" is then prod_j f_j(r). Destroys the prover.
static int composition_eval(int create_rc, bn_sumcheck* sc, const uint32_t* challenges, uint32_t* out) {
	if (create_rc != BN_OK) return create_rc;
	sc->eager = false;
	int rc = BN_OK;
	for (int i = 0; i < sc->num_vars && rc == BN_OK; i++) rc = bn_sumcheck_move_to_next_round(sc, challenges + 4 * (size_t)i);
	uint32_t pts[4 * (kMaxD + 1)];
	if (rc == BN_OK) rc = bn_sumcheck_round_messages(sc, out, pts);
	bn_sumcheck_destroy(sc);
	return rc;
}

extern "C" int bn_multilinear_composition_eval(int device, int num_vars, int d, int transposed, const uint32_t* evals,
                                               const uint32_t* challenges, uint32_t* out) {
	BN_CHECK_ARG(challenges && out, "NULL argument");
	bn_sumcheck* sc = nullptr;
	return composition_eval(bn_sumcheck_create(device, num_vars, d, transposed, evals, &sc), sc, challenges, out);
}

extern "C" int bn_multilinear_composition_eval_device(int device, int num_vars, int d, int transposed, const void* d_evals,
                                                      const uint32_t* challenges, uint32_t* out) {
	BN_CHECK_ARG(challenges && out, "NULL argument");
	bn_sumcheck* sc = nullptr;
	return composition_eval(bn_sumcheck_create_device(device, num_vars, d, transposed, const_cast<void*>(d_evals), 0, &sc), sc, challenges, out);
}
