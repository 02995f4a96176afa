// A stand-in for the HIP functions the failure-injection shim forwards to, so that the shim's bookkeeping can be tested on a
// machine without a GPU (tests/test_failinject_shim.py): allocations come from malloc, streams and events are small heap
// blocks, copies and memsets only count.  standin_counts reports how often each group was reached.
#include <hip/hip_runtime_api.h>

#include <cstdlib>

static unsigned long long g_counts[4];      // creations, releases, copies, memsets
static unsigned long long g_waits;          // stream waits

extern "C" {
void standin_counts(unsigned long long out[4]) { for (int i = 0; i < 4; i++) out[i] = g_counts[i]; }

hipError_t hipMalloc(void** p, size_t n) { g_counts[0]++; *p = std::malloc(n ? n : 1); return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t n, unsigned) { g_counts[0]++; *p = std::malloc(n ? n : 1); return hipSuccess; }
hipError_t hipStreamCreate(hipStream_t* s) { g_counts[0]++; *s = (hipStream_t)std::malloc(8); return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { g_counts[0]++; *s = (hipStream_t)std::malloc(8); return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t* e) { g_counts[0]++; *e = (hipEvent_t)std::malloc(8); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { g_counts[0]++; *e = (hipEvent_t)std::malloc(8); return hipSuccess; }
hipError_t hipFree(void* p) { g_counts[1]++; std::free(p); return hipSuccess; }
hipError_t hipHostFree(void* p) { g_counts[1]++; std::free(p); return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { g_counts[1]++; std::free(s); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { g_counts[1]++; std::free(e); return hipSuccess; }
hipError_t hipMemcpy(void*, const void*, size_t, hipMemcpyKind) { g_counts[2]++; return hipSuccess; }
hipError_t hipMemcpyAsync(void*, const void*, size_t, hipMemcpyKind, hipStream_t) { g_counts[2]++; return hipSuccess; }
hipError_t hipMemcpy2DAsync(void*, size_t, const void*, size_t, size_t, size_t, hipMemcpyKind, hipStream_t) { g_counts[2]++; return hipSuccess; }
hipError_t hipMemcpyPeerAsync(void*, int, const void*, int, size_t, hipStream_t) { g_counts[2]++; return hipSuccess; }
hipError_t hipMemset(void*, int, size_t) { g_counts[3]++; return hipSuccess; }
hipError_t hipMemsetAsync(void*, int, size_t, hipStream_t) { g_counts[3]++; return hipSuccess; }
hipError_t hipMemsetD32Async(hipDeviceptr_t, int, size_t, hipStream_t) { g_counts[3]++; return hipSuccess; }
unsigned long long standin_waits(void) { return g_waits; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t e, unsigned) { g_waits++; return e ? hipSuccess : hipErrorInvalidHandle; }
}
