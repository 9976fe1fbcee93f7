// Pass planner of the eq-indicator expansion (host only; see eq_plan.hpp).
#include "eq_plan.hpp"

namespace bn {

bool eq_plan(int num_vars, int max_levels, EqPlan* plan) {
	if (num_vars < 0 || num_vars > kEqMaxVars || plan == nullptr) return false;
	if (max_levels != 0 && (max_levels < kEqRegLevels || max_levels > kEqTileLevels)) return false;
	const int cap = max_levels ? max_levels : kEqTileLevels;
	EqPlan pl{};
	pl.n_passes = (num_vars + cap - 1) / cap;
	int left = num_vars;  // levels not yet given to a pass, handed out from the last pass back
	for (int p = pl.n_passes - 1; p >= 0; p--) {
		pl.pass[p].levels = left < cap ? left : cap;
		pl.pass[p].shift = num_vars - left;
		left -= pl.pass[p].levels;
	}
	*plan = pl;
	return true;
}

}  // namespace bn
