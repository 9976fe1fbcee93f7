// Pass planning of the BabyBear NTT (host only, bb31_plan.cpp): the digit split of log_n, the pass
// tables the kernels take as arguments, the twiddle table, the list of kernel instances and the
// launch of a pass. No HIP header: this is integer code, and the device side (bb31_ntt.hip) includes
// this file for the constants, the tables and the instance list, so the kernels and the host-side
// sweep (tests/cpp/test_host_asan.cpp) use the same ones.
//
// log_n = m_1 + ... + m_L (the decomposition: bb31_ntt.hip). One pass, the whole array as a single
// tile, for log_n <= kMaxSingleM; above that L = ceil(log_n / kMaxM) digits of log_n / L bits, the
// first log_n % L one more: every digit of a multi-pass plan lies in kMinM..kMaxM.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace bn {
namespace bb31 {

constexpr uint32_t kP = 2013265921u;  // 15 * 2^27 + 1
constexpr int kMaxLogN = 27;
constexpr int kLogCols = 5;
constexpr int kCols = 1 << kLogCols;
constexpr int kMinM = 6;  // digits of a multi-pass plan: kMinM..kMaxM
constexpr int kMaxM = 9;
constexpr int kMaxSingleM = 13;  // largest single tile
constexpr int kThreads = 256;
constexpr int kLoBits = 12;
constexpr int kMaxPasses = (kMaxLogN + kMaxM - 1) / kMaxM;

enum { BB_UPPER = 0, BB_LAST = 1, BB_SINGLE = 2 };

// One pass, passed by value inside the kernel argument: every field is a scalar load from the
// kernarg segment.
struct BbPass {
	int m;          // digit bits of this pass
	int role;       // 0 first/middle (rows stride Mp, 32-column tiles), 1 last, 2 single (whole array)
	int log_mp;     // log2 M_p (columns of the sub-problem; 0 for the last pass)
	int log_sub;    // log2 M_{p-1} (size of the sub-problem)
	int bitrev_in;  // first pass reading a bit-reversed input
	// last pass: k_1 has m_1 bits; (k_2..k_{L-1}) has gbits bits
	int m1, gbits;
	int log_pos[4], log_out[4], mdig[4];  // digits 2..L-1: position stride, output stride, bits
	int ndig;
};

// The passes of a plan in launch order, for an in-order input (a bit-reversed input sets bitrev_in
// on the copy of pass 0 that is launched). False, with *plan untouched, unless 1 <= log_n <= kMaxLogN.
struct BbPlan {
	int log_n, n_passes;
	BbPass pass[kMaxPasses];
};
bool bb_plan(int log_n, BbPlan* plan);

// The twiddle table of a plan, w^e * 2^32 mod p (Montgomery-encoded), w = generator^(2^(log_group_order
// - log_n)): e < 2^log_n in one table, or above kLoBits the table of w^e, e < 2^kLoBits, followed by
// that of w^(e 2^kLoBits), e < 2^(log_n - kLoBits) (w^e is then one Montgomery product of two entries).
constexpr bool bb_hi_split(int log_n) { return log_n > kLoBits; }
std::vector<uint32_t> bb_twiddles(uint32_t generator, int log_group_order, int log_n);

// Every kernel of the transform: bb_pass_r<role, m> for roles 0 and 1; role 2 is the single-tile
// kernel bb_pass, which takes m at run time (the entry's m is the largest it is launched with).
// bb31_ntt.hip instantiates from this list and nothing else, the plan sets the LDS attribute of each
// entry, and bb_plan_launch returns an index into it (tests/cpp/test_host_asan.cpp sweeps log_n
// 1..27: every entry is selected).
struct BbInstance {
	int role, m;
};
constexpr BbInstance kBbInstances[] = {
    {BB_SINGLE, kMaxSingleM}, {BB_UPPER, 6}, {BB_UPPER, 7}, {BB_UPPER, 8}, {BB_UPPER, 9},
    {BB_LAST, 6},             {BB_LAST, 7},  {BB_LAST, 8},  {BB_LAST, 9},
};
constexpr int kBbInstanceCount = (int)(sizeof(kBbInstances) / sizeof(kBbInstances[0]));

// Words of a tile of 2^m rows, and the dynamic LDS of its kernel: the tile, and behind it the
// tile DFT's twiddles w_R^i, i < R / 2
constexpr size_t bb_tile_words(int role, int m) { return (size_t)1 << (role == BB_SINGLE ? m : m + kLogCols); }
constexpr size_t bb_lds_bytes(int role, int m) { return (bb_tile_words(role, m) + ((size_t)1 << m) / 2) * sizeof(uint32_t); }

// One launch of a pass: workgroup (x, y) transforms tile x of transform y of the batch.
struct BbLaunch {
	int instance;  // index into kBbInstances; -1: no instance runs this (role, m)
	size_t tiles, batch, lds;  // grid x, grid y, dynamic LDS bytes
	unsigned threads;
};
// What runs `pass` of a plan of log_n over `batch` transforms. The only place that decides it.
BbLaunch bb_plan_launch(const BbPass& pass, int log_n, size_t batch);

}  // namespace bb31
}  // namespace bn
