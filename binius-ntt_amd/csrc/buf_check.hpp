// Buffer checks of the C-ABI entry points, host only (no HIP include: a CPU program can use them):
// whether two byte ranges overlap and whether a pointer is aligned. Addresses are compared as
// integers, never by pointer arithmetic past an object.
#pragma once

#include <stdint.h>

namespace bn {

// Do [a, a + na) and [b, b + nb) share a byte? A zero-length range overlaps nothing; a range that
// ends at the highest address does not wrap (the ends are compared as distances).
inline bool ranges_overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
	const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
	if (na == 0 || nb == 0) return false;
	return x <= y ? y - x < na : x - y < nb;
}

// `to` is a power of two
inline bool is_aligned(const void* p, uintptr_t to) { return ((uintptr_t)p & (to - 1)) == 0; }

}  // namespace bn
