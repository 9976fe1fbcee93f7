// Round planning of the GF(2^128) sumcheck prover (host only, sc_rounds.cpp): the shape of a round,
// which kernel runs it on which grid with how much LDS, and the development build's measuring
// switches. No HIP header: this is integer code, and the device side (sumcheck.hip) includes this
// file for the constants and the round shape.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "quad_words.hpp"

namespace bn {

constexpr int kScThreads = 256;  // (128: DESIGN.md section 6; 512, one workgroup per CU: 6 % slower on c4)
constexpr int kScMinWG = 512 / kScThreads;  // 2 waves per SIMD (256 VGPRs)
constexpr int kQuadsPerWG = kScThreads / 4;
// Round messages are XOR-accumulated into kAccCopies copies of the (kMaxD + 1) x 4-word point
// set, workgroup b into copy b % kAccCopies, each copy on its own 256-B lines: device-scope
// atomics on one line serialise across the whole grid (about 0.4 ms per c4 run with a single
// copy), spread over 64 lines they overlap. The host XORs the copies.
constexpr int kAccCopies = 64;
constexpr int kAccStride = 64;  // words per copy (>= 4 * (kMaxD + 1))
constexpr int kAccSet = kAccCopies * kAccStride;
// Word kAccStride - 1 of copy 0 counts the finished workgroups; the last one XORs the copies and
// posts the points straight to host-mapped memory, then the round's sequence number in word
// kResSeq (so the host polls one word instead of queueing a copy and synchronising the stream).
constexpr int kAccCount = kAccStride - 1;
constexpr int kResSeq = 4 * (quad::kMaxD + 1);
static_assert(kAccStride > kResSeq, "accumulator copy too small");
constexpr size_t kPostInKernelMaxWG = 64;  // grids up to this post in-kernel (else sc_post)
static_assert(kPostInKernelMaxWG <= (size_t)kAccCopies, "an in-kernel posting grid stores one copy per workgroup");
constexpr size_t kHexMaxItems = 8192;   // launches up to this many items use 16-lane products
constexpr size_t kWideMaxItems = 1024;  // ... and up to this many the 64-lane product
// sc_fold_pair: LDS rows of 64 words padded to 68, 64 lane rows per wave, two lanes per item
constexpr int kPairRowWords = 68;
constexpr int kPairWaveWords = 64 * kPairRowWords;
constexpr int kPairItemsPerWG = kScThreads / 2;
constexpr size_t kPairMinItems = 384 * (size_t)kPairItemsPerWG;
// sc_server: one workgroup of 12 waves, three per SIMD (the wide product fits 168 VGPRs)
constexpr int kSrvThreads = 768;
constexpr int kSrvG = 64;  // wide_mul: latency is all that counts there (a few items per round)
constexpr int kSrvGroups = kSrvThreads / kSrvG;
constexpr size_t kServerMaxCur = 512;  // the server takes over at this many evaluations per column

// A round on `cur` (a power of two) evaluations per column of a degree-d composition. While
// cur >= 64 a butterfly pairs whole batches (mode 0); below that the one batch pairs bit-lanes
// (mode 1), and cur == 1 is the final evaluation (mode 2). constexpr: callable from device code as
// it is.
struct ScShape {
	int d;
	int mode;        // 0 big, 1 in-batch pairs, 2 single element
	size_t n_pairs;  // batch pairs (big mode) or 1
	size_t hb;       // batch distance of a pair (big mode)
	int h;           // element distance of a pair inside the batch (mode 1)
	int kmax;        // points 0..kmax
};
constexpr ScShape sc_shape(size_t cur, int d) {
	return cur >= 64 ? ScShape{d, 0, cur / 64, cur / 64, 0, d} : cur >= 2 ? ScShape{d, 1, 1, 0, (int)(cur / 2), d} : ScShape{d, 2, 1, 0, 0, 0};
}

// Every kernel that takes dynamic LDS: sc_messages<mode, G> and sc_fold<mode, G> on G-lane
// products, and the two big-mode folds. Nothing else is instantiated.
enum class ScKernel { Messages0G4, Messages0G16, Messages0G64, Messages1G64, Messages2G64, Fold0G16, Fold1G16, FoldCoal, FoldPair };
constexpr int kScKernelCount = (int)ScKernel::FoldPair + 1;

// Development build (BN_DEV) only, read from the environment once per prover by sc_dev_knobs(); the
// product build has the defaults below and reads nothing. They measure, or choose among the
// product kernels:
//   BN_SC_DBG             bit 0 = synthetic operands instead of column loads, bit 1 = no products,
//                         bit 2 = no k-multiples, bit 3 = no parity reduction (wrong results: the
//                         kernels' memory-and-LDS floors, tools/sc_dbg_trace.sh)
//   BN_SC_HEX_MAX         kHexMaxItems, BN_SC_WIDE_MAX kWideMaxItems (big-mode messages move
//                         between the 4-, 16- and 64-lane kernels; a big-mode fold that leaves
//                         the coalesced kernels runs on 16 lanes)
//   BN_SC_POST_MAX        kPostInKernelMaxWG (at most kAccCopies)
//   BN_SC_FOLD_PAIR=0     sc_fold_coal where sc_fold_pair would run
//   BN_SC_SERVER_MAX_CUR  kServerMaxCur (0: no round server)
//   BN_SC_TIMING          the server stamps its phases; the host prints them per round
struct ScKnobs {
	int dbg = 0;
	size_t hex_max = kHexMaxItems, wide_max = kWideMaxItems, post_max = kPostInKernelMaxWG;
	bool fold_pair = true;
	size_t server_max_cur = kServerMaxCur;
	bool timing = false;
};
ScKnobs sc_dev_knobs();

// One launch: one item per lane group of G lanes (fold: (column, pair); messages: (pair, point)).
struct ScLaunch {
	ScKernel kernel;
	int G;            // lanes per product (2: sc_fold_pair)
	size_t items, per_wg, grid;
	int threads;
	size_t lds;       // dynamic LDS bytes
	int post;         // ScArgs::post: the last workgroup posts the points
	bool post_kernel; // sc_post follows (messages on a grid too large to post in-kernel)
};
ScLaunch sc_plan_launch(const ScShape& s, bool fold, int skip1, const ScKnobs& k);

// the largest dynamic LDS request of any ScKernel, and sc_server's
size_t sc_max_lds_bytes();
size_t srv_lds_bytes();

}  // namespace bn
