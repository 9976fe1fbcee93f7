// Shared host-side plumbing for the C-ABI: status codes, thread-local last error,
// HIP error checking that reports instead of aborting.
#pragma once

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <string>

#include "binius_ntt_amd.h"

namespace bn {

void set_error(const char* fmt, ...);
void clear_error();

// The calling thread's current device set to `dev` for a scope, and put back on every way out of it.
struct DeviceScope {
	int prev = -1;
	hipError_t err = hipSuccess;  // of the switch to `dev`
	explicit DeviceScope(int dev) {
		if (hipGetDevice(&prev) != hipSuccess) prev = -1;
		if (prev != dev) err = hipSetDevice(dev);
	}
	~DeviceScope() {
		int cur = -1;
		if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
	}
	DeviceScope(const DeviceScope&) = delete;
	DeviceScope& operator=(const DeviceScope&) = delete;
};

}  // namespace bn

// a DeviceScope for the rest of the block; a failed switch returns BN_ERR_HIP
#define BN_DEVICE_SCOPE(dev)                                                                                  \
	::bn::DeviceScope device_scope_(dev);                                                                     \
	if (device_scope_.err != hipSuccess)                                                                      \
	BN_FAIL(BN_ERR_HIP, "hipSetDevice(%d) failed: %s", (int)(dev), hipGetErrorString(device_scope_.err))

#define BN_FAIL(code, ...)             \
	do {                               \
		::bn::set_error(__VA_ARGS__);  \
		return (code);                 \
	} while (0)

#define BN_HIP(call)                                                                                   \
	do {                                                                                               \
		hipError_t e_ = (call);                                                                        \
		if (e_ != hipSuccess) {                                                                        \
			::bn::set_error("%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_));       \
			return BN_ERR_HIP;                                                                         \
		}                                                                                              \
	} while (0)

#define BN_CHECK_ARG(cond, ...)                      \
	do {                                             \
		if (!(cond)) BN_FAIL(BN_ERR_INVALID, __VA_ARGS__); \
	} while (0)
