/*
 * binius_ntt_amd.h — the C-ABI drop-in boundary of the MI355X (gfx950) binary-tower /
 * additive-NTT engine. Plain pointers and sizes only; every entry point returns an int
 * status (0 = BN_OK) and never aborts; bn_last_error() describes the last failure on the
 * calling thread.
 *
 * Each entry point names the reference interface it replaces (shourovrm/binius-NTT,
 * paths relative to its repository root). The C++ mirror of the reference surface
 * (AdditiveNTT<T,P>, NTTData, Sumcheck<N,d,T>, ...) lives in binius-ntt_amd/host/ulvt and
 * calls only these functions.
 *
 * Element layouts (bit-exact with the reference):
 *   GF(2^32) element  : one uint32_t.
 *   GF(2^128) element : four uint32_t limbs, little-endian (limb 0 = bits 0..31),
 *                       as src/ulvt/sumcheck/test/utils/bigints.cu:6-13.
 *   bitsliced block   : 128 uint32_t words; word i holds bit i of 32 consecutive GF(2^128)
 *                       elements, element e in bit e (src/ulvt/utils/bitslicing.cuh:32-47).
 */
#ifndef BINIUS_NTT_AMD_H
#define BINIUS_NTT_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
	BN_OK = 0,
	BN_ERR_INVALID = 1,     /* bad argument (reference: ASSERT / apply() returning false) */
	BN_ERR_HIP = 2,         /* HIP runtime failure other than an allocation (reference: CUDA_CHECK, common.cuh:18-29) */
	BN_ERR_UNSUPPORTED = 3, /* valid in the reference surface but not built here */
	BN_ERR_ALLOC = 4        /* device or host allocation failure: every device allocation of a plan, a
	                           prover or a host call's staging reports it, with the size in bn_last_error() */
};
/* The *_host calls are synchronous on every path: when one returns, with whatever status, no copy
 * from or to the caller's buffers is still queued. */

/* Description of the last error on this thread ("" if none). */
const char* bn_last_error(void);
/* Library version string. */
const char* bn_version(void);

/* Replaces bool check_gpu_capabilities() (src/ulvt/utils/common.cu:6-43): returns 1 if a
 * gfx950 device with enough LDS for the kernels is visible, else 0. */
int bn_check_gpu_capabilities(void);

/* ------------------------------------------------------------------------------------
 * Additive NTT (src/ulvt/ntt/additive_ntt.cuh, src/ulvt/ntt/nttconf.cuh)
 * ------------------------------------------------------------------------------------ */
typedef struct bn_antt_plan bn_antt_plan;

/* Replaces AdditiveNTTConf<T,P>(log_h, log_rate) (nttconf.cuh:55-60) + the AdditiveNTT
 * constructor (additive_ntt.cuh:178-199): validates 1 <= log_h, 0 <= log_rate <= 4,
 * log_h + log_rate <= field_bits (and <= 32: every twiddle must lie in GF(2^32)),
 * precomputes the normalised subspace evaluations on the host and stages them on
 * `device`. field_bits is 32 (T=uint32_t, P=FanPaarTowerField<5>) or 128 (GF(2^128)). */
int bn_antt_plan_create(int device, int field_bits, int log_h, int log_rate, bn_antt_plan** plan);
/* Replaces ~AdditiveNTT (additive_ntt.cuh:267-270). NULL is accepted. */
int bn_antt_plan_destroy(bn_antt_plan* plan);

/* Replaces bool AdditiveNTT::apply(const NTTData<T>& in, NTTData<T>& out)
 * (additive_ntt.cuh:201-265): host buffers, synchronous. in_elems must equal 2^log_h
 * (the reference returns false otherwise: here BN_ERR_INVALID with no other effect);
 * `out` receives 2^(log_h+log_rate) elements, coset-major. */
int bn_antt_forward_host(bn_antt_plan* plan, const void* in, size_t in_elems, void* out);

/* Device-resident entry (no reference counterpart; used by benchmarks, batched and
 * multi-GPU callers): `batch` independent transforms, transform b reads
 * d_in + b*2^log_h elements and writes d_out + b*2^(log_h+log_rate) elements.
 * d_in and d_out must not overlap. Asynchronous on `stream` (a hipStream_t, may be 0). */
int bn_antt_forward_device(bn_antt_plan* plan, const void* d_in, void* d_out, size_t batch, void* stream);

/* Inverse transform on the device (no reference counterpart: the reference transforms in one
 * direction only). With F_c(x) block `coset` of bn_antt_forward_device's output for input x
 * (elements [coset*2^log_h, (coset+1)*2^log_h)), writes the unique x with F_c(x) = y: evaluations
 * on one coset, in order, back to novel-basis coefficients, bit-exact. `batch` independent
 * transforms on the same coset; transform b reads d_in + b*2^log_h elements and writes
 * d_out + b*2^log_h elements. d_in is not written; d_in and d_out must not overlap;
 * 0 <= coset < 2^log_rate (BN_ERR_INVALID otherwise, nothing is launched). Asynchronous on
 * `stream`. Variant 0 runs compact tiles, variants 1, 4 and 5 bitsliced LDS tiles. */
int bn_antt_inverse_device(bn_antt_plan* plan, const void* d_in, void* d_out, int coset, size_t batch, void* stream);
/* The same with host buffers (no reference counterpart), synchronous, staged through the plan's
 * own stream like bn_antt_forward_host. in_elems must equal 2^log_h (BN_ERR_INVALID with no other
 * effect otherwise); `out` receives 2^log_h elements. */
int bn_antt_inverse_host(bn_antt_plan* plan, const void* in, size_t in_elems, int coset, void* out);

/* FRI-Binius codeword folding (Diamond-Posen; no reference counterpart), GF(2^128) plans only
 * (BN_ERR_UNSUPPORTED for a 32-bit plan: the challenges live in GF(2^128)). Bit-exact.
 * The codeword at round i is 2^log_rate blocks, coset-major, of m_i = 2^(log_h-i) compact elements;
 * round 0 is the output of bn_antt_forward_device. One round i with challenge r maps block c from
 * m_i to m_i/2 elements: for j < m_i/2, with t the transform's own twiddle of stage i, block j,
 * coset c (the XOR of s[i][k] over the set bits k < log_h+log_rate-1-i of (c << (log_h-1-i)) | j,
 * a GF(2^32) value that multiplies limb by limb),
 *   u = in[c][2j], v = in[c][2j+1]
 *   v' = u ^ v                         (odd part)
 *   u' = u ^ t*v'                      (even part)
 *   out[c][j] = u' ^ r*(u' ^ v')       ((1-r) u' + r v', full GF(2^128) product)
 * A call folds rounds round .. round+arity-1 with challenges r_0 .. r_{arity-1} (r_0 first) in one
 * launch: the input is read once and the output written once. Folding the codeword of x through all
 * log_h rounds leaves 2^log_rate equal elements, the multilinear extension of x at r (bit i of the
 * index pairs with r_i): bn_multilinear_composition_eval(x, log_h, 1, challenges reversed).
 * `challenges` is host memory, arity x 4 words, read before the call returns (passed to the kernel
 * by value: no staging copy, the call stays asynchronous on `stream`). `batch` codewords share the
 * challenges: codeword b reads d_in + b*2^(log_h+log_rate-round) elements and writes
 * d_out + b*2^(log_h+log_rate-round-arity) elements. d_in is not written.
 * BN_ERR_INVALID, with nothing launched: a NULL plan, buffer or challenges, round < 0, arity outside
 * [1, 8], round + arity > log_h, batch == 0, overlapping d_in and d_out ranges. */
int bn_antt_fri_fold_device(bn_antt_plan* plan, const void* d_in, void* d_out, int round, int arity,
                            const uint32_t* challenges, size_t batch, void* stream);
/* The same on one codeword in host memory, synchronous, through the plan's own stream like
 * bn_antt_inverse_host. in_elems must equal 2^(log_h+log_rate-round) (BN_ERR_INVALID with no other
 * effect otherwise); `out` receives 2^(log_h+log_rate-round-arity) elements. */
int bn_antt_fri_fold_host(bn_antt_plan* plan, const void* in, size_t in_elems, int round, int arity,
                          const uint32_t* challenges, void* out);
/* The verifier's fold of one opened leaf (host only: no plan, no device).
 * out = element `index` of the output of bn_antt_fri_fold_device(round, arity) for a (log_h, log_rate)
 * GF(2^128) plan, computed from the 2^arity input elements [index << arity, (index+1) << arity) in
 * `leaf` (the leaf bn_merkle_open_device returns for that index at log_leaf_elems = arity) and the
 * arity challenges. Level l pairs leaf elements 2p, 2p+1 by the per-pair rule with the twiddle of
 * stage round+l at the global pair index (index << (arity-1-l)) | p (low log_h+log_rate-1-round-l
 * bits). Host arithmetic; bit-exact with the device fold. The subspace table is kept per thread
 * while (log_h, log_rate) repeats. BN_ERR_INVALID: NULL pointer, parameters
 * outside bn_antt_plan_create's / the fold's ranges, index >= 2^(log_h+log_rate-round-arity). */
int bn_antt_fri_fold_leaf(int log_h, int log_rate, int round, int arity, uint64_t index,
                          const uint32_t* leaf, const uint32_t* challenges, uint32_t* out);

/* Copies the plan's normalised subspace-evaluation table s[i][j] (GF(2^32) values,
 * log_h rows x (log_h+log_rate-1) columns, row-major) to host memory. */
int bn_antt_get_subspace_evals(const bn_antt_plan* plan, uint32_t* out, size_t out_words);

/* Plan introspection: 0 log_h, 1 log_rate, 2 field_bits, 3 device, 4 kernel variant. */
int bn_antt_plan_query(const bn_antt_plan* plan, int what, int64_t* value);
/* Kernel selection, the analogue of choosing AdditiveNTT vs ModifiedAdditiveNTT
 * (src/ulvt/ntt/modified_antt.cuh:223-427, benchmark_antt.cu): 0 = compact tiles with the twiddle
 * recomputed per butterfly from the subspace table (the reference kernel's scheme), 1 = bitsliced
 * LDS tiles with host-tabulated twiddle contributions, 4 = bitsliced register tiles (three to four
 * waves per SIMD) on every pass, 5 = variant 4 for the passes whose twiddles all lie in GF(2^8)
 * and variant 1 for the others (default when log_h >= 12). Other values
 * return BN_ERR_INVALID. Variants 1, 4 and 5 need log_h >= 12; results are identical. */
int bn_antt_plan_set_variant(bn_antt_plan* plan, int variant);

/* Profiling hook for bench.py: records hipEvents around every kernel launch of the next
 * bn_antt_forward_device call on its stream and returns per-launch-kind mean durations. */
int bn_antt_set_event_timing(bn_antt_plan* plan, int enable);
int bn_antt_get_event_timing(bn_antt_plan* plan, float* ms_per_kind, int max_kinds, int* n_kinds);
/* Profiling (no reference counterpart; bench.py's roofline): every pass of the transform is
 * launched `reps` times back to back on `stream` between two hipEvents, giving its steady-state
 * duration per launch in ms_per_pass[pass]. d_out's contents are meaningless afterwards (passes
 * are re-applied to their own output; their cost does not depend on the values). Variants
 * 1, 4 and 5. Synchronous. */
int bn_antt_time_passes(bn_antt_plan* plan, const void* d_in, void* d_out, size_t batch, int reps,
                        void* stream, float* ms_per_pass, int max_passes, int* n_passes);
/* Profiling (no reference counterpart): the demangled name of the kernel that pass `pass` of the
 * plan's current variant launches, as rocprofv3 reports it (e.g. "void bn::antt_bs_pass<4, 2, 32,
 * false>(bn::BsParams)"), so committed counter summaries can be matched to the launches exactly.
 * BN_ERR_UNSUPPORTED for variant 0. */
int bn_antt_pass_kernel_name(bn_antt_plan* plan, int pass, char* buf, size_t cap);
/* Test hook (no reference counterpart; host only: no plan, no device): the twiddle tables of the
 * in-word stages 0..4 of the bitsliced bottom pass (variants 1 and 5) of a (log_h, log_rate)
 * transform, log_h >= 12, so that a test can rebuild every twiddle from them. The first four
 * words give the layout, so a caller hard-codes none of it (a 1024-word buffer is ample):
 *   words, B, O, R                   words written in all; block bits per tile (7), table rows
 *                                    for fixed bits (20) and for coset bits (8)
 *   n_outer, ob[O]                   the index bits (>= 12) fixed per tile, ascending
 *   then for s = 0..4, 32 + B + O + R + 1 words:
 *     pat2[32]  word i = bit i of the bit-lane part of the twiddle: at stage s bit-lane bits
 *               0..s-1 are index bits 0..s-1 (no twiddle part), bit-lane bits s..3 index bits
 *               s+1..4 and bit-lane bit 4 index bit 11
 *     twt[B]    contribution of index bit 5 + m (the lane owns bits 5..10; bit 11 is in pat2)
 *     two[O]    contribution of fixed index bit ob[m]
 *     twc[R]    contribution of coset bit c
 *     field     8/16/32: the sub-field holding every twiddle of the stage
 * BN_ERR_UNSUPPORTED for log_h < 12, BN_ERR_INVALID if out_words is too small. */
int bn_antt_inword_tables(int log_h, int log_rate, uint32_t* out, size_t out_words);
/* Test hook (no reference counterpart; host only: no plan, no device): the sub-field class that
 * the register-tile pass table carries for every stage above the bottom pass of a (log_h, log_rate)
 * transform, out[s - 12] for stage s = 12 .. log_h - 1: the smallest of 0 (every twiddle of the
 * stage is zero), 2, 4, 8, 16, 32 bits that holds every twiddle of the stage. The first pass's
 * GF(2^8) register-tile kernels pick the stage's multiply circuit by it (0: none, 2: bsm1x16_fma_tw,
 * 4: bsm2x8_fma_tw, 8: bsm3x4_fma_tw); every other kernel rounds 0 / 2 / 4 up to 8.
 * BN_ERR_UNSUPPORTED for log_h < 12, BN_ERR_INVALID if n < log_h - 12. */
int bn_antt_stage_classes(int log_h, int log_rate, int32_t* out, size_t n);

/* ------------------------------------------------------------------------------------
 * Binary tower field arithmetic (src/ulvt/finite_fields/)
 * ------------------------------------------------------------------------------------ */
/* Elementwise GF(2^128) product of compact vectors, n elements, device pointers.
 * Semantics of tower_height_7_mul (src/ulvt/sumcheck/test/utils/tower_7_mul.cu:4-20). Any n;
 * alias-safe (d_out == d_a or d_out == d_b). Runs on the bitsliced quad-lane product behind
 * in-LDS bit transposes (78 KB of dynamic LDS per work-group). */
int bn_gf128_mul_device(const void* d_a, const void* d_b, void* d_out, size_t n, void* stream);
/* Same on bitsliced 128-word blocks: multiply_unrolled<7> (circuit_generator/unrolled/
 * binary_tower_unrolled7.cu), n_blocks blocks of 32 products each. Alias-safe (d_out == d_a). */
int bn_gf128_mul_bitsliced_device(const void* d_a, const void* d_b, void* d_out, size_t n_blocks, void* stream);
/* Elementwise GF(2^32) product (FanPaarTowerField<5>::multiply, binary_tower.cuh:113-115). */
int bn_gf32_mul_device(const void* d_a, const void* d_b, void* d_out, size_t n, void* stream);
/* Register-resident repeat-loop microbenchmarks in the style of bitsliced_repeat
 * (src/ulvt/finite_fields/tests/profiling/kernels/bitsliced_repeat.cu:5-32):
 * kind 0 = compact GF(2^128), kind 1 = bitsliced GF(2^128) (32 products per lane-block,
 * multiply_unrolled<7> per lane), kind 2 = bitsliced GF(2^128) on the quad-lane product of the
 * sumcheck (one 32-product block per quad of lanes).
 * Each of `threads` lanes (kinds 0, 1) or blocks (kind 2) performs `iters` dependent products;
 * d_state holds threads*4 (kind 0) or threads*128 (kinds 1, 2) words, updated in place, and
 * d_operand holds the multipliers in the same shape. */
int bn_gf128_mul_repeat_device(int kind, void* d_state, const void* d_operand, size_t threads, int iters, void* stream);

/* ------------------------------------------------------------------------------------
 * Bitslicing (src/ulvt/utils/bitslicing.cuh:89-105)
 * ------------------------------------------------------------------------------------ */
/* In-place compact -> bitsliced (untranspose == 0) or bitsliced -> compact (untranspose != 0)
 * over n_blocks 128-word blocks. Replaces transpose_kernel / untranspose_kernel. */
int bn_bitslice_device(void* d_buf, size_t n_blocks, int untranspose, void* stream);

/* ------------------------------------------------------------------------------------
 * Bit-reversal permutation of a device-resident GF(2^128) column (no reference counterpart): the
 * data movement that lets the sumcheck (highest variable first) and the FRI fold (lowest index bit
 * first) bind the variables in the same order
 * ------------------------------------------------------------------------------------ */
/* out[b*2^n + rev_n(x)] = in[b*2^n + x], x < 2^n, b < batch: compact GF(2^128) elements (16 B),
 * rev_n = the n-bit reversal of the index. bitsliced != 0: each transform's output is then in the
 * layout of bn_bitslice_device (needs log_n >= 5), i.e. the call equals the compact call followed
 * by bn_bitslice_device on d_out; the buffer is a data_is_transposed sumcheck column as it is.
 * The index is split hi (6 bits) | mid | lo (6 bits): a work-group moves the 2^12 elements of one
 * value of mid through LDS, reading 64 runs of 1 KiB and writing 64 runs of 1 KiB, so every global
 * access is whole 128-byte lines (log_n <= 1 is one device-to-device copy).
 * d_in is not written; d_in and d_out must not overlap. Allocates nothing, asynchronous on
 * `stream`, current device, all indexing 64-bit. 0 <= log_n <= 30. BN_ERR_INVALID with nothing
 * launched: NULL or misaligned (16 B) buffer, log_n out of range, bitsliced with log_n < 5,
 * batch == 0 or batch*2^log_n > 2^32 elements, overlapping ranges. */
int bn_bit_reverse_device(const void* d_in, void* d_out, int log_n, size_t batch, int bitsliced, void* stream);
/* The same on one transform in host memory (2^log_n x 4 words each way), synchronous, staged through
 * a buffer on `device` that lives for the call. */
int bn_bit_reverse_host(int device, const uint32_t* in, int log_n, int bitsliced, uint32_t* out);
/* Test hook: the same with the tile's run length forced to 2^tile_log elements, 1..6 (0: default;
 * other values BN_ERR_INVALID), so that multi-tile plans run at 2^4 .. 2^13 elements. Results are
 * identical. */
int bn_bit_reverse_device_split(const void* d_in, void* d_out, int log_n, size_t batch, int bitsliced,
                                int tile_log, void* stream);

/* ------------------------------------------------------------------------------------
 * Field primitives beside the hot path (src/ulvt/finite_fields)
 * ------------------------------------------------------------------------------------ */
/* Replaces multiply_unrolled<HEIGHT>(a, b, dst) (circuit_generator/unrolled/
 * binary_tower_unrolled.cuh:4-5): 32 bitsliced GF(2^(2^height)) products, 2^height words per
 * operand (word i = bit i of the 32 elements). Host computation; alias-safe (dst may be a or b,
 * as core.cu:21 uses it). 2 <= height <= 7. */
int bn_multiply_unrolled(int height, const uint32_t* a, const uint32_t* b, uint32_t* dst);
/* Device batch of the same: nblocks blocks of 2^height words per operand. Async on `stream`. */
int bn_multiply_unrolled_device(int height, const void* a, const void* b, void* dst, size_t nblocks, void* stream);
/* Test hook (no reference counterpart): runs generated circuit `circuit` (0..13, the order of
 * bitsliced_gen.hpp: bsm2_mul, bsm3_mul, bsm3x4_fma_tw, bsm3x4_mul_acc, bsm4_mul, bsm4x2_fma_tw,
 * bsm4x2_mul_acc, bsm5_mul, bsm5_fma_tw, bsm5_mul_acc, bsm6_mul, bsm7_mul, bsm5_mul_w,
 * bsm6_fma_w2) on the device, one 32-product block per lane, operands as that circuit
 * documents. d_out is read first by the accumulate forms. Per-lane compact twiddles: one word per
 * block in d_b. Wave-uniform ones (bsm5_mul_w: one word, bsm6_fma_w2: two words): one entry
 * per 64 consecutive blocks, passed to the circuit through readfirstlane as the kernels do.
 * Buffers must not overlap. BN_ERR_INVALID for an unknown id, a NULL pointer or more than 2^30
 * blocks; n_blocks == 0 launches nothing. Asynchronous on `stream`. */
int bn_circuit_device(int circuit, const void* d_a, const void* d_b, void* d_out, size_t n_blocks, void* stream);
/* Replaces mul_binary_tower_32b_simd<HEIGHT>(a, b) (binary_tower_simd.cuh:77-127): the words as
 * 32/2^height packed GF(2^(2^height)) elements, multiplied lane by lane. 0 <= height <= 5. */
int bn_mul_binary_tower_32b_simd(int height, uint32_t a, uint32_t b, uint32_t* out);
/* Replaces interleave_32b<HEIGHT>(a, b) -> (c, d) and xor_adjacent_32b<HEIGHT>(a)
 * (binary_tower_simd.cuh:129-150); 0 <= height <= 4. */
int bn_interleave_32b(int height, uint32_t a, uint32_t b, uint32_t* c, uint32_t* d);
int bn_xor_adjacent_32b(int height, uint32_t a, uint32_t* out);
/* Device batch over n words: op 0 = mul_binary_tower_32b_simd (c = a*b), 1 = interleave_32b
 * ((c, d) from (a, b)), 2 = xor_adjacent_32b (c from a; b, d unused). Async on `stream`. */
int bn_packed32_device(int op, int height, const void* a, const void* b, void* c, void* d, size_t n, void* stream);

/* ------------------------------------------------------------------------------------
 * Sumcheck over GF(2^128) (src/ulvt/sumcheck/sumcheck.cuh:10-301)
 * ------------------------------------------------------------------------------------ */
typedef struct bn_sumcheck bn_sumcheck;

/* Replaces Sumcheck<NUM_VARS, COMPOSITION_SIZE, DATA_IS_TRANSPOSED>(evals, benchmarking)
 * (sumcheck.cuh:82-126). evals: composition_size columns of 4*2^num_vars words each,
 * column-major; compact when data_is_transposed == 0 (converted on the device), bitsliced
 * 128-word blocks otherwise. 1 <= num_vars <= 30 (>= 5 for bitsliced input),
 * 1 <= composition_size <= 8.
 * The host copy is made synchronously. */
int bn_sumcheck_create(int device, int num_vars, int composition_size, int data_is_transposed,
                       const uint32_t* evals, bn_sumcheck** sc);
/* bn_sumcheck_create in the reference constructor's two timed phases (sumcheck.cuh:88-124:
 * start_before_memcpy, start_before_transpose, start_raw): _staged allocates and copies the host
 * columns (synchronous, the "Memcpy" phase) and leaves compact input untransposed;
 * bn_sumcheck_prepare runs the device bit-transpose and synchronises (the "Transpose" phase; a
 * no-op for bitsliced input or a prepared prover). A staged prover used without prepare is
 * prepared by its first round call. */
int bn_sumcheck_create_staged(int device, int num_vars, int composition_size, int data_is_transposed,
                              const uint32_t* evals, bn_sumcheck** sc);
int bn_sumcheck_prepare(bn_sumcheck* sc);
/* As above but from device memory already holding the columns (no host copy). The buffer
 * is copied into the prover's own storage unless take_ownership != 0, in which case the
 * prover folds it in place and frees it with hipFree on destroy (so it must come from
 * hipMalloc). The copy (or first use) runs on the prover's own stream, ordered after the work
 * queued on the legacy default stream; a producer on any other stream must have completed
 * (the Python mirror synchronises the tensor's current stream first). */
int bn_sumcheck_create_device(int device, int num_vars, int composition_size, int data_is_transposed,
                              void* d_evals, int take_ownership, bn_sumcheck** sc);
/* Replaces Sumcheck::this_round_messages(sum, points) (sumcheck.cuh:130-246):
 * sum[4], points[4*(composition_size+1)] (round polynomial at 0..d). Blocks until the round's
 * points are posted (the calling thread polls host memory). */
int bn_sumcheck_round_messages(bn_sumcheck* sc, uint32_t* sum, uint32_t* points);
/* Replaces Sumcheck::move_to_next_round(challenge) (sumcheck.cuh:248-300). Asynchronous: queues
 * the fold and the next round's messages kernel on the prover's stream and returns. */
int bn_sumcheck_move_to_next_round(bn_sumcheck* sc, const uint32_t* challenge);
/* Current round (0 .. num_vars). */
int bn_sumcheck_round(const bn_sumcheck* sc, int* round);
/* Multi-GPU sharding: this prover holds shard `rank` of `world` (interleaved by 32-element
 * batch index); round messages are then partial and must be XOR-combined across ranks by
 * the caller (the Python/RCCL layer does allgather + XOR). world must be a power of two
 * with 32*world <= 2^num_vars. Must be called before the first round. */
int bn_sumcheck_set_shard(bn_sumcheck* sc, int rank, int world);
/* A shard prover built directly from this rank's share (no reference counterpart): d_local
 * holds the bitsliced batches b with b mod world == rank, in order (4*2^num_vars/world words per
 * column, columns back to back). The copy is ordered after the work queued on `stream` (a
 * hipStream_t; NULL = default stream). Equivalent to bn_sumcheck_create_device on the whole
 * input followed by bn_sumcheck_set_shard(rank, world), without any rank holding the whole. */
int bn_sumcheck_create_shard_device(int device, int num_vars, int composition_size, int rank, int world,
                                    const void* d_local, void* stream, bn_sumcheck** sc);
/* Sharded endgame (no reference counterpart; the reference's analogue is the hand-over to the
 * CPU at 32 evaluations, sumcheck.cuh:283-297): once every shard is down to one 32-element
 * batch (*flag = 1), folds pair elements of different ranks. Each rank exports its batch
 * (composition_size * 128 words), the caller all-gathers them rank-major and every rank
 * imports the concatenation; the prover then continues unsharded. */
int bn_sumcheck_needs_gather(const bn_sumcheck* sc, int* flag);
/* Device-resident round exchange (no reference counterpart): every later round-messages kernel also
 * writes the round's raw point words into d_words (device memory, >= 4*(8+1)+1 words, or NULL to
 * stop): words 0 .. 4*(composition_size+1)-1 = the kernel's points 0..d (p(1) zero when it was not
 * computed), word 36 = flags: bit 0 set if p(1) was left out (the caller then has p(1) = claim + p(0)
 * and sum = claim with the round's claim, which for XOR-combined shards is the global one; clear:
 * sum = p(0) + p(1)); bit 1 set for the last call (one evaluation left: words 0-3 are the sum,
 * prod_j f_j(r), and there are no points). The words are written before the posted sequence number, so they are complete
 * once bn_sumcheck_round_messages has returned; consumers on other streams order themselves after
 * the prover's stream (bn_sumcheck_stream) to read them. A prover with a sink never starts the
 * resident round server; while a server started earlier runs (an unsharded prover's last rounds),
 * setting a sink returns BN_ERR_INVALID. */
int bn_sumcheck_set_message_sink(bn_sumcheck* sc, void* d_words);
/* Sharded drivers with a message sink: replaces bn_sumcheck_round_messages without waiting for the
 * round. Makes sure the round's messages kernel is queued on the prover's stream and returns; the
 * raw points and flags reach the sink in stream order, so a consumer orders itself after
 * bn_sumcheck_stream (e.g. enqueues its collective there) and never polls the host. The caller
 * then holds the round's global points: the next round skips p(1) when the prover derives it
 * (sink word 36 bit 0) and the caller completes it from the global claim. Once used, the rounds
 * up to the endgame gather must all be read this way. BN_ERR_INVALID while a round server runs. */
int bn_sumcheck_round_messages_sink(bn_sumcheck* sc);
int bn_sumcheck_stream(const bn_sumcheck* sc, void** stream);
int bn_sumcheck_export_shard(const bn_sumcheck* sc, uint32_t* out, size_t out_words);
int bn_sumcheck_import_gathered(bn_sumcheck* sc, const uint32_t* words, size_t n_words, int world);
int bn_sumcheck_destroy(bn_sumcheck* sc);

/* ------------------------------------------------------------------------------------
 * Verifier side of the sumcheck (src/ulvt/sumcheck/test/verifier.cu)
 * ------------------------------------------------------------------------------------ */
/* Replaces evaluate_multilinear_composition(evals, challenges, num_vars, composition_size)
 * (verifier.cu:88-107, with evaluate_multilinear_given_point :33-86 and lagrange_basis_eval,
 * kernel/verifier_kernel.cu:4-37): out = prod_j sum_x f_j(x) prod_v (x_v ? r[n-1-v] : 1 + r[n-1-v]),
 * i.e. every column folded at the challenges (highest variable first), multiplied together.
 * Computed on `device` by the sumcheck fold kernels. evals as bn_sumcheck_create (host memory,
 * compact or bitsliced); challenges: num_vars x 4 words. Synchronous. */
int bn_multilinear_composition_eval(int device, int num_vars, int composition_size, int data_is_transposed,
                                    const uint32_t* evals, const uint32_t* challenges, uint32_t* out);
/* Same with the columns already in device memory (left untouched). */
int bn_multilinear_composition_eval_device(int device, int num_vars, int composition_size, int data_is_transposed,
                                           const void* d_evals, const uint32_t* challenges, uint32_t* out);
/* Replaces evaluate_univariate_given_points(challenge, points, num_points) (verifier.cu:9-31):
 * Lagrange interpolation through (k, points[k]), k = 0..num_points-1 (tower elements), evaluated
 * at `challenge`. Host arithmetic; 1 <= num_points <= 16. */
int bn_sumcheck_interpolate(const uint32_t* points, int num_points, const uint32_t* challenge, uint32_t* out);

/* ------------------------------------------------------------------------------------
 * The eq-indicator (tensor) expansion of a point (no reference counterpart): the column that
 * turns a sumcheck into a zerocheck or an evaluation claim
 * ------------------------------------------------------------------------------------ */
/* Writes E[x] = scale * prod_{i<n} ( bit_{n-1-i}(x) ? r_i : 1 ^ r_i ), x = 0 .. 2^n - 1, n = num_vars,
 * to device memory, bit-exact. The convention is bn_multilinear_composition_eval's: `challenges` is
 * num_vars x 4 words of host memory, r_i = challenges[i], highest variable first (challenges[i] pairs
 * with index bit n-1-i), so that for scale = 1
 *   XOR_x f[x]*E[x] == bn_multilinear_composition_eval(f, n, 1, challenges).
 * d_out receives 2^n elements: compact (16 bytes each) when bitsliced == 0, else bitsliced 128-word
 * blocks in element order, the layout of bn_bitslice_device and of a data_is_transposed sumcheck
 * column (the buffer can be handed to bn_sumcheck_create_device as a column as it is). `scale` is 4
 * words of host memory, or NULL for 1 (a shard driver passes the table over the variables it does
 * not hold). `challenges` and `scale` are read before the call returns (passed to the kernels by
 * value: no staging copy and no synchronisation, the call is asynchronous on `stream`). One level
 * takes the table A over the k highest variables to k + 1 (hi = A[y]*r_k, lo = A[y] ^ hi): 2^n - 1
 * products in all, each by a launch constant. The levels run in place in d_out in passes of at
 * most 12 (30 = 6 + 12 + 12) and the call allocates nothing; d_out's contents between the passes are
 * partial tables. Bitsliced output runs the in-place bit transpose behind the last pass. Runs on
 * the current device, as bn_gf128_mul_device does.
 * 0 <= num_vars <= 30, and >= 5 when bitsliced; all indexing is 64-bit. BN_ERR_INVALID, with nothing
 * launched: num_vars out of range, a NULL d_out, NULL challenges with num_vars > 0, bitsliced with
 * num_vars < 5. */
int bn_eq_expand_device(int num_vars, const uint32_t* challenges, const uint32_t* scale, void* d_out, int bitsliced,
                        void* stream);
/* The same into host memory (2^num_vars x 4 words), synchronous, staged through a buffer on
 * `device` that lives for the call. */
int bn_eq_expand_host(int device, int num_vars, const uint32_t* challenges, const uint32_t* scale, int bitsliced,
                      uint32_t* out);
/* out = prod_{i<num_vars} (a_i*b_i ^ (1 ^ a_i)*(1 ^ b_i)): the value of the expansion of a at the
 * point b (symmetric; the order of the variables does not matter as long as a and b agree), which a
 * verifier needs for a zerocheck's last claim. a, b: num_vars x 4 words. Host arithmetic;
 * 0 <= num_vars <= 128. */
int bn_eq_eval(int num_vars, const uint32_t* a, const uint32_t* b, uint32_t* out);
/* Test hook: bn_eq_expand_device with the per-pass level cap forced to max_levels, 3 .. 12 (0: the
 * default, 12; other values BN_ERR_INVALID), so that three- and four-pass plans run at 2^9 - 2^13
 * elements. Results are identical. */
int bn_eq_expand_device_split(int num_vars, const uint32_t* challenges, const uint32_t* scale, void* d_out,
                              int bitsliced, int max_levels, void* stream);
/* Test hook (host only: no device): the host planner's split of num_vars levels at the cap
 * max_levels (as above), levels[p] of pass p, first pass first; *n_passes passes (none for
 * num_vars == 0). The last pass has min(num_vars, cap) levels, the passes before it cap each and the
 * first the remainder. BN_ERR_INVALID if an argument is out of range or cap < *n_passes. */
int bn_eq_expand_passes(int num_vars, int max_levels, int32_t* levels, size_t cap, int* n_passes);

/* ------------------------------------------------------------------------------------
 * Ring-switching for GF(2) witnesses (no reference counterpart; Diamond-Posen, "Polylogarithmic Proofs
 * for Multilinears over Binary Towers", section 4): the reduction from "t(r) = s", t a multilinear with
 * 2^l bits and r in GF(2^128)^l, to a sumcheck over the packed column t'[w] = sum_v t[128 w + v] beta_v
 * (2^(l-7) elements) that the FRI-Binius opening finishes. beta_v is the element whose only set bit is
 * bit v: bit v % 32 of word v / 32. With r_low = r[0:7], r_high = r[7:l] and E[w] = eq(r_high, w)
 * (r_high,j pairs with bit j of w):
 *   partial evaluations  s^_v = XOR over w with bit_v(t'[w]) = 1 of E[w], v = 0 .. 127
 *   row check            s == sum_v eq(r_low, v) s^_v                    (r_low,i pairs with bit i of v)
 *   batching             B[u] = eq(r'', u), r'' in GF(2^128)^7           (r''_i pairs with bit i of u)
 *   sumcheck claim       s_0 = sum_u B[u] s^row_u, s^row_u = sum_v bit_u(s^_v) beta_v
 *   sumcheck column      A[w] = XOR over u with bit_u(E[w]) = 1 of B[u]; sum_w A[w] t'[w] = s_0
 *   last claim           A~(rho) = sum_u B[u] e_u, e = prod_j (1 (x) (1 ^ rho_j) + r_high,j (x) 1)
 * Every result is bit-exact.
 * ------------------------------------------------------------------------------------ */
/* The partial evaluations of two bitsliced columns of 2^log_n elements (128-word blocks, the layout of
 * bn_bitslice_device and of a data_is_transposed sumcheck column), both in the same element order:
 * d_out receives 128 compact elements (2 KiB; it need not be initialised, the call zeroes it on
 * `stream`). Per block a GF(2) matrix product acc[v][u] ^= T[v] & E[u] (16 384 lane-operations per 32
 * elements); work-groups of eight waves take contiguous runs of blocks and combine with atomicXor.
 * Neither input is written. Allocates nothing, asynchronous on `stream`, current device, all indexing
 * 64-bit. 5 <= log_n <= 30. BN_ERR_INVALID with nothing launched: NULL or misaligned (16 B) buffer,
 * log_n out of range, d_out inside an input. */
int bn_rs_partial_evals_device(const void* d_packed, const void* d_eq, int log_n, void* d_out, void* stream);
/* The same on host memory (2^log_n x 4 words per column, bitsliced blocks; out: 128 x 4 words),
 * synchronous, staged through a buffer on `device` that lives for the call. */
int bn_rs_partial_evals_host(int device, const uint32_t* packed, const uint32_t* eq, int log_n, uint32_t* out);
/* Test hook: the same with at most max_blocks_per_group blocks per work-group (0: the default), so
 * that several work-groups, the last one short, reduce into one result at 2^6 .. 2^13 elements.
 * Results are identical. */
int bn_rs_partial_evals_device_split(const void* d_packed, const void* d_eq, int log_n, void* d_out,
                                     size_t max_blocks_per_group, void* stream);
/* A GF(2)-linear map of GF(2^128) applied to every element: out[w] = XOR over u with bit_u(in[w]) = 1
 * of matrix[u]. `matrix` is 128 x 4 words of host memory, read before the call returns (passed to the
 * kernel by value). bitsliced == 0: n >= 1 compact elements. bitsliced != 0: n 128-word blocks, in and
 * out in the layout of bn_bitslice_device. In place (d_out == d_in) is allowed; any other overlap is
 * rejected. The compact kernel looks every byte of the element up in one of 16 tables of 256 entries
 * in LDS (64 KiB, built per work-group); bitsliced blocks run it between the two bit transposes, in
 * place in d_out. Allocates nothing, asynchronous on `stream`, current device. BN_ERR_INVALID with
 * nothing launched: NULL argument, misaligned (16 B) buffer, n == 0 or above 2^32 elements,
 * partially overlapping ranges. */
int bn_gf128_linear_map_device(const void* d_in, void* d_out, size_t n, const uint32_t* matrix, int bitsliced,
                               void* stream);
/* The same on host memory, synchronous, staged through a buffer on `device` that lives for the call. */
int bn_gf128_linear_map_host(int device, const uint32_t* in, size_t n, const uint32_t* matrix, int bitsliced,
                             uint32_t* out);
/* The verifier's arithmetic (host only: no plan, no device).
 * bn_rs_batch_table: out[u] = B[u], 128 x 4 words, from r2 = r'' (7 x 4 words); also the `matrix` the
 * prover passes to bn_gf128_linear_map_device. */
int bn_rs_batch_table(const uint32_t* r2, uint32_t* out);
/* out = sum_v eq(r_low, v) s^_v: the right-hand side of the row check. shat 128 x 4, r_low 7 x 4. */
int bn_rs_row_check(const uint32_t* shat, const uint32_t* r_low, uint32_t* out);
/* out = s_0, the sumcheck's claim, from s^ and r''. */
int bn_rs_sumcheck_claim(const uint32_t* shat, const uint32_t* r2, uint32_t* out);
/* out = A~(rho): 256 products and one 128 x 128 bit-matrix application per variable. r_high and rho are
 * n x 4 words (NULL allowed for n == 0), 0 <= n <= 121. */
int bn_rs_eq_eval(int n, const uint32_t* r_high, const uint32_t* rho, const uint32_t* r2, uint32_t* out);

/* ------------------------------------------------------------------------------------
 * SHA-256 Merkle commitment of a device-resident GF(2^128) codeword and its query openings (no
 * reference counterpart): the step between bn_antt_forward_device and bn_antt_fri_fold_device, and
 * between one fold and the next. Every result is bit-exact.
 *
 * The rule. L = log_leaves, a = log_leaf_elems (0 .. 8), L + a <= 30.
 *   Input        2^L leaves. Leaf j is the 2^a consecutive compact elements [j << a, (j + 1) << a) of one
 *                flat buffer: the elements one bn_antt_fri_fold_device call of arity a folds into
 *                output element j (round + arity <= log_h there, so a leaf never straddles a coset
 *                block).
 *   Leaf digest  SHA-256 (FIPS 180-4, with its padding) of the leaf's 16 << a bytes as they lie in
 *                memory (four little-endian uint32 limbs per element, limb 0 first).
 *   Node digest  one SHA-256 compression, no padding and no length block: the state starts at the
 *                standard initial value, the 64-byte block is left || right, the digest is the eight
 *                state words after the feed-forward addition, each big-endian. Two all-zero children
 *                give da5698be17b9b46962335799779fbeca8ce5d491c0d26243bafef9ea1837a9d8. With L = 0 the
 *                root is the leaf digest.
 *   Tree buffer  2^(L+1) - 1 digests of 32 bytes. Row 0 (the 2^L leaf digests) first, then row 1
 *                (2^(L-1) nodes), ..., the root last at digest index 2^(L+1) - 2. Row h starts at digest
 *                index 2^(L+1) - 2^(L-h+1); node k of row h + 1 is node(row_h[2k], row_h[2k+1]).
 *   Opening      of leaf j: the leaf's 16 << a bytes, then L sibling digests from the bottom up, the
 *                one at row h being row_h[(j >> h) ^ 1]: 16 * 2^a + 32 * L bytes.
 * All element and byte offsets are 64-bit. Device buffers must be 16-byte aligned.
 * ------------------------------------------------------------------------------------ */
/* The two sizes (host only): *n = 2^(L+1) - 1 digests of the tree buffer (0 <= L <= 30); *bytes of one
 * opening record. */
int bn_merkle_tree_digests(int log_leaves, size_t* n);
int bn_merkle_open_bytes(int log_leaves, int log_leaf_elems, size_t* bytes);
/* *index = the digest index of node 0 of `row` (0 <= row <= log_leaves) in the tree buffer (host only). */
int bn_merkle_row_offset(int log_leaves, int row, size_t* index);
/* Commits to the 2^(L+a) elements at d_data: fills d_tree (32 * (2^(L+1) - 1) bytes) by the rule
 * above. Asynchronous on `stream`; allocates nothing and uses no scratch buffer: the rows are written
 * into d_tree and read back from it by the later passes (a leaf pass of 256 leaves a work-group that
 * goes on to rows 1 and 2, row passes of three rows each, and one work-group that finishes the tree
 * from a row of at most 2^9 digests), stream order being the only synchronisation. d_data is not
 * written. Runs on the current device.
 * BN_ERR_INVALID, with nothing launched and no buffer touched: a NULL or misaligned pointer,
 * log_leaf_elems outside [0, 8], log_leaves < 0 or log_leaves + log_leaf_elems > 30, overlapping
 * d_data and d_tree ranges. */
int bn_merkle_commit_device(const void* d_data, int log_leaves, int log_leaf_elems, void* d_tree, void* stream);
/* Test hook: the same with the planner's rows-per-pass cap forced to max_rows, 1 .. 3, for every
 * pass, the tail included (0: the default, three rows for the leaf and row passes and up to nine for
 * the tail; other values BN_ERR_INVALID), so that a tree of 2^10 leaves has several row passes.
 * Results are identical. */
int bn_merkle_commit_device_split(const void* d_data, int log_leaves, int log_leaf_elems, void* d_tree, int max_rows,
                                  void* stream);
/* The same on host buffers (data: 2^(L+a) x 4 words, tree: 32 * (2^(L+1) - 1) bytes), synchronous,
 * staged through a buffer on `device` that lives for the call. */
int bn_merkle_commit_host(int device, const uint32_t* data, int log_leaves, int log_leaf_elems, uint8_t* tree);
/* Writes the opening record of leaf d_indices[q] at d_out + q * record bytes, q = 0 .. n_queries - 1.
 * d_indices is device memory (uint32), so the call needs no staging copy and is asynchronous on
 * `stream`; queued behind the commitment on the same stream it needs no synchronisation. An index
 * >= 2^L gives an all-zero record and reads nothing out of range; duplicates are allowed.
 * BN_ERR_INVALID, with nothing launched: as for the commitment, n_queries == 0 (or above 2^40 bytes
 * of records), d_out overlapping d_data, d_tree or d_indices. */
int bn_merkle_open_device(const void* d_data, const void* d_tree, int log_leaves, int log_leaf_elems,
                          const uint32_t* d_indices, size_t n_queries, void* d_out, void* stream);
/* What a verifier needs (host integer code, no device): the digest of a leaf of 16 << log_leaf_elems
 * bytes, the digest of a node, and the check of an opening record of leaf `index` against a root
 * (*ok = 1 if the path hashes to root32, else 0, also for index >= 2^L). */
int bn_merkle_hash_leaf(const void* leaf, int log_leaf_elems, uint8_t* out32);
int bn_merkle_hash_node(const uint8_t* left32, const uint8_t* right32, uint8_t* out32);
int bn_merkle_verify(const uint8_t* root32, int log_leaves, int log_leaf_elems, uint64_t index, const void* record, int* ok);
/* Test hook (host only): the planner's split of the rows 0 .. L at the cap max_rows (as above). Pass
 * p is out[3p .. 3p+2] = kind (0 leaf pass, 1 row pass, 2 tail), the first row it writes, the number
 * of rows it writes; *n_passes passes, at most 32. One leaf pass first; the tail, if any, last.
 * BN_ERR_INVALID if an argument is out of range or cap < *n_passes. */
int bn_merkle_commit_passes(int log_leaves, int log_leaf_elems, int max_rows, int32_t* out, size_t cap, int* n_passes);


/* ------------------------------------------------------------------------------------
 * BabyBear radix-2 NTT, the prime-field sibling path (src/ulvt/ntt/gpuntt.cuh,
 * NTTConfRad2 in src/ulvt/ntt/nttconf.cuh:25-47, BB31 = risc0::Fp,
 * src/ulvt/finite_fields/risc0_baby_bear.h:40-190). Elements are uint32_t holding the
 * canonical value (BB31::asUInt32(); inputs are reduced mod p = 15*2^27+1 as BB31(r) does).
 * The transform is the natural-order DFT X[k] = sum_j x[j] w^(jk), w = g^(2^(log_group-log_n)).
 * Raw risc0 Fp words (Montgomery form, val = x * 2^32 mod p, the bytes of NTTData<BB31> in the
 * reference) are accepted as well: the transform is linear and multiplies data only by
 * Montgomery-encoded twiddles, so Montgomery words (< p) in give the reference's Montgomery
 * words out (tests/test_bb31.py::test_gpu_montgomery_words_in_montgomery_words_out).
 * ------------------------------------------------------------------------------------ */
typedef struct bn_bb31_ntt_plan bn_bb31_ntt_plan;

/* Replaces NTTConfRad2<BB31>(generator, log_group_order, log_inp_size) (nttconf.cuh:31-38:
 * 1 <= log_n <= 27, log_group_order >= log_n) + the NTT<BB31> constructor (gpuntt.cuh:128-146,
 * twiddle precomputation). generator is a canonical value (BB31(137) -> 137). */
int bn_bb31_ntt_plan_create(int device, uint32_t generator, int log_group_order, int log_n, bn_bb31_ntt_plan** plan);
int bn_bb31_ntt_plan_destroy(bn_bb31_ntt_plan* plan);

/* Replaces NTT<BB31>::apply(input, output) (gpuntt.cuh:150-183): host in -> host out,
 * synchronous, output in order. in_bit_reversed = 1 for NTTData::order == BIT_REVERSED (the
 * input is used as stored), 0 for IN_ORDER. BN_ERR_INVALID if in_elems != 2^log_n (the
 * reference ASSERTs). */
int bn_bb31_ntt_forward_host(bn_bb31_ntt_plan* plan, const uint32_t* in, size_t in_elems, uint32_t* out,
                             int in_bit_reversed);

/* Device-resident, asynchronous on `stream` (hipStream_t, NULL = default): batch transforms of
 * 2^log_n words each, contiguous; d_in and d_out must not overlap. Multi-pass sizes
 * (log_n >= 14) stage their data in the plan's scratch buffer, so a plan is used by one stream
 * at a time (and not concurrently with forward_host); use one plan per stream. */
int bn_bb31_ntt_forward_device(bn_bb31_ntt_plan* plan, const uint32_t* d_in, uint32_t* d_out, size_t batch,
                               int in_bit_reversed, void* stream);


/* ------------------------------------------------------------------------------------
 * QM31 sumcheck, the prime-field sibling of the GF(2^128) sumcheck
 * (src/ulvt/prime_field_sumcheck/sumcheck.cuh:8-96, core/kernels.cu:5-77). A QM31 element
 * is 4 uint32_t M31 words (lo.a, lo.b, hi.a, hi.b), canonical (< 2^31 - 1) on output.
 * ------------------------------------------------------------------------------------ */
typedef struct bn_qm31_sumcheck bn_qm31_sumcheck;

/* Replaces Sumcheck<NUM_VARS>(evals, benchmarking) (sumcheck.cuh:24-44): evals = column 0 then
 * column 1, 2^num_vars QM31 each (8 * 2^num_vars words); 1 <= num_vars <= 28 (the reference
 * instantiates 1, 20, 24, 28). */
int bn_qm31_sumcheck_create(int device, int num_vars, const uint32_t* evals, bn_qm31_sumcheck** sc);
/* Replaces this_round_messages<BLOCKS, THREADS>(points) (sumcheck.cuh:46-86): points 0, 1, 2
 * (12 words). */
int bn_qm31_sumcheck_round_messages(bn_qm31_sumcheck* sc, uint32_t* points);
/* Replaces fold<BLOCKS, THREADS>(challenge) (sumcheck.cuh:88-96). */
int bn_qm31_sumcheck_fold(bn_qm31_sumcheck* sc, const uint32_t* challenge);
/* After the last fold: the two remaining values f0(r), f1(r) (8 words). */
int bn_qm31_sumcheck_final_values(bn_qm31_sumcheck* sc, uint32_t* out);
int bn_qm31_sumcheck_destroy(bn_qm31_sumcheck* sc);

#ifdef __cplusplus
}
#endif
#endif
