// Planner of the bit-reversal permutation (host only; see bitrev_plan.hpp).
#include "bitrev_plan.hpp"

namespace bn {

bool bitrev_plan(int log_n, uint64_t batch, int tile_log, BitrevPlan* plan) {
	if (log_n < 0 || log_n > kBitrevMaxLog || plan == nullptr) return false;
	if (tile_log < 0 || tile_log > kBitrevTileLog) return false;
	if (batch == 0 || batch > (kBitrevMaxElems >> log_n)) return false;
	const int cap = tile_log ? tile_log : kBitrevTileLog;
	BitrevPlan pl{};
	pl.n = log_n;
	pl.q = log_n / 2 < cap ? log_n / 2 : cap;
	pl.m = log_n - 2 * pl.q;
	pl.n_tiles = batch << pl.m;
	*plan = pl;
	return true;
}

}  // namespace bn
