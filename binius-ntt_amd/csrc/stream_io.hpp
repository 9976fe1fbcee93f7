// Streaming (non-temporal) 16-byte global accesses for data a kernel touches once: the NTT passes'
// tiles, the eq expansion's last pass, the Merkle leaf pass's codeword.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bn {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 ld_stream(const uint32_t* p) {
	const u32x4 v = __builtin_nontemporal_load((const u32x4*)p);
	return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st_stream(uint32_t* p, uint4 g) {
	u32x4 v;
	v.x = g.x;
	v.y = g.y;
	v.z = g.z;
	v.w = g.w;
	__builtin_nontemporal_store(v, (u32x4*)p);
}

}  // namespace bn
