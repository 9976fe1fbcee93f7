// AdditiveNTT<T, P> (src/ulvt/ntt/additive_ntt.cuh:175-319) over the C-ABI.
//
//   AdditiveNTT<uint32_t, FanPaarTowerField<5>>            GF(2^32), as the reference
//   AdditiveNTT<unsigned __int128, FanPaarTowerField<7>>   GF(2^128) (4 little-endian u32 limbs)
//
// Construction builds the plan (subspace table precompute + device staging, the reference ctor
// 178-199); apply() has the reference's host semantics (201-265): returns false, with no other
// effect, unless in.size == 2^log_h and in.order == IN_ORDER; otherwise writes 2^(log_h+log_rate)
// elements coset-major into out, sets out.order = IN_ORDER and returns after a full sync.
#pragma once

#include <cstdint>
#include <utility>

#include "../finite_fields/binary_tower.hpp"
#include "../utils/common.hpp"
#include "nttconf.hpp"

template <typename T, typename P>
class AdditiveNTT {
	static_assert(sizeof(T) * 8 == P::N_BITS(), "element type must match the field policy");

public:
	explicit AdditiveNTT(const AdditiveNTTConf<T, P>& conf, int device = 0) : ntt_conf(conf) {
		ulvt::bn_check(bn_antt_plan_create(device, (int)P::N_BITS(), conf.log_h, conf.log_rate, &plan));
	}
	AdditiveNTT(const AdditiveNTT&) = delete;
	AdditiveNTT& operator=(const AdditiveNTT&) = delete;
	~AdditiveNTT() { bn_antt_plan_destroy(plan); }

	bool apply(const NTTData<T>& input, NTTData<T>& output) {
		if (input.size != ((size_t)1 << ntt_conf.log_h) || input.order != DataOrder::IN_ORDER) return false;
		if (output.size < ((size_t)1 << (ntt_conf.log_h + ntt_conf.log_rate))) return false;
		ulvt::bn_check(bn_antt_forward_host(plan, input.data.get(), input.size, output.data.get()));
		output.order = DataOrder::IN_ORDER;
		return true;
	}

	// Device-resident transforms (no reference counterpart): `batch` transforms, asynchronous
	// on `stream` (a hipStream_t).
	void forward_device(const void* d_in, void* d_out, size_t batch = 1, void* stream = nullptr) {
		ulvt::bn_check(bn_antt_forward_device(plan, d_in, d_out, batch, stream));
	}

	// Inverse (no reference counterpart): evaluations on coset `coset` (block `coset` of apply()'s
	// output) back to coefficients. Returns false, with no other effect, unless input.size ==
	// 2^log_h, input.order == IN_ORDER and output holds 2^log_h elements; otherwise writes 2^log_h
	// elements, sets output.order = IN_ORDER and returns after a full sync.
	bool inverse(const NTTData<T>& input, NTTData<T>& output, int coset = 0) {
		if (input.size != ((size_t)1 << ntt_conf.log_h) || input.order != DataOrder::IN_ORDER) return false;
		if (output.size < ((size_t)1 << ntt_conf.log_h)) return false;
		ulvt::bn_check(bn_antt_inverse_host(plan, input.data.get(), input.size, coset, output.data.get()));
		output.order = DataOrder::IN_ORDER;
		return true;
	}

	// `batch` device-resident inverse transforms on one coset, asynchronous on `stream`.
	void inverse_device(const void* d_in, void* d_out, int coset = 0, size_t batch = 1, void* stream = nullptr) {
		ulvt::bn_check(bn_antt_inverse_device(plan, d_in, d_out, coset, batch, stream));
	}

	// FRI-Binius fold (no reference counterpart; GF(2^128) plans): the codeword of round `round`
	// (round 0: apply()'s output) folded `arity` times with challenges[0 .. 4*arity), challenges[0..3]
	// first. Returns false, with no other effect, unless input.size == 2^(log_h+log_rate-round),
	// input.order == IN_ORDER, 1 <= arity <= log_h - round and output holds input.size >> arity
	// elements; otherwise writes that many elements, sets output.order = IN_ORDER and returns after a
	// full sync.
	bool fri_fold(const NTTData<T>& input, NTTData<T>& output, int round, const uint32_t* challenges, int arity) {
		if (round < 0 || arity < 1 || round + arity > ntt_conf.log_h) return false;
		if (input.size != ((size_t)1 << (ntt_conf.log_h + ntt_conf.log_rate - round)) || input.order != DataOrder::IN_ORDER)
			return false;
		if (output.size < (input.size >> arity)) return false;
		ulvt::bn_check(bn_antt_fri_fold_host(plan, input.data.get(), input.size, round, arity, challenges, output.data.get()));
		output.order = DataOrder::IN_ORDER;
		return true;
	}

	// `batch` device-resident folds sharing the challenges (host memory, read before the call
	// returns), one launch, asynchronous on `stream`.
	void fri_fold_device(const void* d_in, void* d_out, int round, const uint32_t* challenges, int arity, size_t batch = 1,
	                     void* stream = nullptr) {
		ulvt::bn_check(bn_antt_fri_fold_device(plan, d_in, d_out, round, arity, challenges, batch, stream));
	}

	// The verifier's fold of one opened leaf (host arithmetic: no device work, the plan gives only
	// log_h and log_rate): element `index` of fri_fold(round, arity)'s output from the 2^arity input
	// elements [index << arity, (index + 1) << arity) in `leaf`. Bit-exact with the device fold.
	T fri_fold_leaf(int round, uint64_t index, const T* leaf, const uint32_t* challenges, int arity) const {
		static_assert(sizeof(T) == 16 || sizeof(T) == 4, "GF(2^128) or GF(2^32) elements");
		if (sizeof(T) != 16) throw ulvt::BnError(BN_ERR_UNSUPPORTED, "binius-ntt-amd: fri_fold_leaf is built for GF(2^128) plans");
		T out{};
		ulvt::bn_check(bn_antt_fri_fold_leaf(ntt_conf.log_h, ntt_conf.log_rate, round, arity, index, (const uint32_t*)leaf, challenges,
		                                     (uint32_t*)&out));
		return out;
	}

	// 0: compact tiles, per-butterfly twiddles (default for log_h < 12); 1: bitsliced LDS tiles;
	// 4: bitsliced register tiles; 5: 4 for the GF(2^8)-twiddle passes, 1 for the others (default
	// for log_h >= 12)
	void set_variant(int variant) { ulvt::bn_check(bn_antt_plan_set_variant(plan, variant)); }

	const AdditiveNTTConf<T, P>& conf() const { return ntt_conf; }

private:
	AdditiveNTTConf<T, P> ntt_conf;
	bn_antt_plan* plan = nullptr;
};
