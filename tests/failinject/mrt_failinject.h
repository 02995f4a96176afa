// Failure injection for the host library's resource paths (test infrastructure, never the product).
//
// The Makefile compiles the host .cpp files a second time with this header force-included (-include) and links them, the
// unchanged kernel objects and mrt_failinject.cpp into lib/libmyraytracer_amd_failinject.so.  In that build the library's own
// calls of the six resource creators and the four releasers go through the shim with their source site, and its copies and
// memsets are range-checked against the live device allocations.  tests/test_gpu_failure_paths.py drives it.  Its stream waits
// go through the shim too, which can drop one of them (tests/test_gpu_stream_order.py).
#pragma once
#ifdef MRT_FAILINJECT_SHIM
#include <hip/hip_runtime_api.h>        // (the shim itself is plain host C++)
#else
#include <hip/hip_runtime.h>
#endif
#include <stddef.h>
#include <stdint.h>

extern "C" {
// ---- the routed calls (file / line: the call's site in the library) ----
hipError_t mrt_fi_malloc(const char* file, int line, void** p, size_t bytes);
hipError_t mrt_fi_host_malloc(const char* file, int line, void** p, size_t bytes, unsigned flags);
hipError_t mrt_fi_stream_create(const char* file, int line, hipStream_t* s, int with_flags, unsigned flags);
hipError_t mrt_fi_event_create(const char* file, int line, hipEvent_t* e, int with_flags, unsigned flags);
hipError_t mrt_fi_free(const char* file, int line, void* p);
hipError_t mrt_fi_host_free(const char* file, int line, void* p);
hipError_t mrt_fi_stream_destroy(const char* file, int line, hipStream_t s);
hipError_t mrt_fi_event_destroy(const char* file, int line, hipEvent_t e);
hipError_t mrt_fi_memcpy(const char* file, int line, void* dst, const void* src, size_t bytes, hipMemcpyKind kind);
hipError_t mrt_fi_memcpy_async(const char* file, int line, void* dst, const void* src, size_t bytes, hipMemcpyKind kind,
                               hipStream_t stream);
hipError_t mrt_fi_memcpy2d_async(const char* file, int line, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width,
                                 size_t height, hipMemcpyKind kind, hipStream_t stream);
hipError_t mrt_fi_memcpy_peer_async(const char* file, int line, void* dst, int dst_dev, const void* src, int src_dev, size_t bytes,
                                    hipStream_t stream);
hipError_t mrt_fi_memset(const char* file, int line, void* dst, int value, size_t bytes);
hipError_t mrt_fi_memset_async(const char* file, int line, void* dst, int value, size_t bytes, hipStream_t stream);
hipError_t mrt_fi_memset_d32_async(const char* file, int line, hipDeviceptr_t dst, int value, size_t count, hipStream_t stream);
hipError_t mrt_fi_stream_wait_event(const char* file, int line, hipStream_t stream, hipEvent_t event, unsigned flags);

// ---- the tests' interface ----
// The n-th creator call from now on (n >= 1) is refused without reaching the runtime; the count restarts at zero.  One shot.
void mrt_fi_arm(uint64_t n);
void mrt_fi_disarm(void);                       // no refusal pending; the count keeps running
uint64_t mrt_fi_calls(void);                    // creator calls since the last arm / reset
// 1 if the armed refusal has happened (site: "file.cpp:line hipName", truncated to cap), else 0
int mrt_fi_fired(char* site, size_t cap);
// the distinct creator sites seen since the last reset, "file.cpp:line hipName" one per line, sorted; returns the bytes needed
size_t mrt_fi_sites(char* buf, size_t cap);
void mrt_fi_live(uint64_t out[4]);              // live {device allocations, pinned allocations, streams, events}
// what went wrong since the last reset, one per line; returns how many (the text is truncated to cap)
size_t mrt_fi_violations(char* buf, size_t cap);
void mrt_fi_reset(void);                        // forget the sites, the violations and the counts; disarm.  Live resources stay.
// The stream waits (hipStreamWaitEvent), counted apart from the creators (tests/order_walks.py).  The n-th from now on (n >= 1)
// returns hipSuccess without reaching the runtime -- the wait is dropped, nothing is refused; the count restarts at zero.  One
// shot; n == 0 only counts.  mrt_fi_reset forgets these too.
void mrt_fi_skip_wait(uint64_t n);
uint64_t mrt_fi_waits(void);                    // stream waits since the last mrt_fi_skip_wait / reset
// 1 if the wait has been dropped (site: "file.cpp:line hipStreamWaitEvent", truncated to cap), else 0
int mrt_fi_skipped(char* site, size_t cap);
// the distinct stream-wait sites seen since the last reset, one per line, sorted; returns the bytes needed
size_t mrt_fi_wait_sites(char* buf, size_t cap);
}

#ifndef MRT_FAILINJECT_SHIM
template <class T> static inline hipError_t mrt_fi_malloc_t(const char* f, int l, T** p, size_t n) { return mrt_fi_malloc(f, l, (void**)p, n); }
template <class T> static inline hipError_t mrt_fi_host_malloc_t(const char* f, int l, T** p, size_t n, unsigned flags = hipHostMallocDefault) {
    return mrt_fi_host_malloc(f, l, (void**)p, n, flags);
}
#define hipMalloc(...) mrt_fi_malloc_t(__FILE__, __LINE__, __VA_ARGS__)
#define hipHostMalloc(...) mrt_fi_host_malloc_t(__FILE__, __LINE__, __VA_ARGS__)
#define hipStreamCreate(s) mrt_fi_stream_create(__FILE__, __LINE__, (s), 0, 0u)
#define hipStreamCreateWithFlags(s, flags) mrt_fi_stream_create(__FILE__, __LINE__, (s), 1, (flags))
#define hipEventCreate(e) mrt_fi_event_create(__FILE__, __LINE__, (e), 0, 0u)
#define hipEventCreateWithFlags(e, flags) mrt_fi_event_create(__FILE__, __LINE__, (e), 1, (flags))
#define hipFree(p) mrt_fi_free(__FILE__, __LINE__, (p))
#define hipHostFree(p) mrt_fi_host_free(__FILE__, __LINE__, (p))
#define hipStreamDestroy(s) mrt_fi_stream_destroy(__FILE__, __LINE__, (s))
#define hipEventDestroy(e) mrt_fi_event_destroy(__FILE__, __LINE__, (e))
#define hipMemcpy(...) mrt_fi_memcpy(__FILE__, __LINE__, __VA_ARGS__)
#define hipMemcpyAsync(...) mrt_fi_memcpy_async(__FILE__, __LINE__, __VA_ARGS__)
#define hipMemcpy2DAsync(...) mrt_fi_memcpy2d_async(__FILE__, __LINE__, __VA_ARGS__)
#define hipMemcpyPeerAsync(...) mrt_fi_memcpy_peer_async(__FILE__, __LINE__, __VA_ARGS__)
#define hipMemset(...) mrt_fi_memset(__FILE__, __LINE__, __VA_ARGS__)
#define hipMemsetAsync(...) mrt_fi_memset_async(__FILE__, __LINE__, __VA_ARGS__)
#define hipMemsetD32Async(...) mrt_fi_memset_d32_async(__FILE__, __LINE__, __VA_ARGS__)
#define hipStreamWaitEvent(...) mrt_fi_stream_wait_event(__FILE__, __LINE__, __VA_ARGS__)
#endif
