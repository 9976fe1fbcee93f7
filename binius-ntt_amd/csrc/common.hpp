// Shared host-side plumbing for the C-ABI: status codes, thread-local last error,
// HIP error checking that reports instead of aborting, the device guard, the owners of a device
// allocation and of a per-call stream, and the staged (host in, device, host out) round trip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <utility>

#include "binius_ntt_amd.h"
#include "buf_check.hpp"

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

// The library's one device allocation: BN_ERR_ALLOC, with the size in the message, when it fails.
int dev_alloc(void** p, size_t bytes);
template <class T>
int dev_alloc(T** p, size_t bytes) {
	return dev_alloc((void**)p, bytes);
}

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

// the bytes a *_device transform reads and the bytes it writes must share none (buf_check.hpp)
#define BN_CHECK_IO_DISJOINT(d_in, in_bytes, d_out, out_bytes) \
	BN_CHECK_ARG(!::bn::ranges_overlap((d_in), (in_bytes), (d_out), (out_bytes)), "d_in and d_out must not overlap")

namespace bn {

// A list of kernel instances as kernels: fns[i] = At<i>::fn() over the whole list (nullptr where At
// leaves an entry to another file)
template <template <int> class At, size_t... I>
const void* instance_table(int instance, std::index_sequence<I...>) {
	static const void* const fns[] = {At<(int)I>::fn()...};
	return fns[instance];
}

// A device allocation that is freed on the way out unless release() hands it to a plan or prover.
struct DevBuf {
	void* p = nullptr;
	DevBuf() = default;
	DevBuf(const DevBuf&) = delete;
	DevBuf& operator=(const DevBuf&) = delete;
	~DevBuf() {
		if (p) (void)hipFree(p);
	}
	int alloc(size_t bytes) { return dev_alloc(&p, bytes); }
	void* release() { return std::exchange(p, nullptr); }
};

// A non-blocking stream that lives for one call.
struct CallStream {
	hipStream_t s = nullptr;
	CallStream() = default;
	CallStream(const CallStream&) = delete;
	CallStream& operator=(const CallStream&) = delete;
	~CallStream() {
		if (s) (void)hipStreamDestroy(s);
	}
	int create() {
		BN_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
		return BN_OK;
	}
};

// Host in -> device -> host out, synchronous, on `st`: in_bytes of `in` are copied to d_in (nothing
// when in_bytes is 0), `launch(st)` queues the work and returns a BN_* code, out_bytes of d_out are
// copied to `out` (d_in and d_out may lie in one allocation). The first failure stops the queueing
// and is the one reported; the stream is synchronised on every path, so on return it is idle: the
// device buffers may be freed and the caller's host memory is touched no more.
template <class Launch>
int staged_call(hipStream_t st, const void* in, void* d_in, size_t in_bytes, const void* d_out, void* out, size_t out_bytes,
                Launch launch) {
	const int rc = [&]() -> int {
		if (in_bytes) BN_HIP(hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, st));
		if (int r = launch(st)) return r;
		BN_HIP(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, st));
		return BN_OK;
	}();
	const hipError_t es = hipStreamSynchronize(st);
	if (rc != BN_OK) return rc;
	if (es != hipSuccess) BN_FAIL(BN_ERR_HIP, "hipStreamSynchronize after a staged call -> %s", hipGetErrorString(es));
	return BN_OK;
}

}  // namespace bn
