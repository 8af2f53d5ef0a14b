// tools/device_mem_check/hip/hip_runtime.h -- host stand-in for the HIP calls srsran_amd/csrc/device_mem.h makes, so
// its ownership logic runs under the host sanitizers: allocations come from malloc (a leak or a double free is the
// sanitizer's to report), every call is counted, and the fail_alloc-th hipMalloc from now fails.
#pragma once
#include <stdlib.h>
#include <string.h>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1 };
typedef void* hipStream_t;

struct StubHip {
  int allocs = 0, frees = 0, copies = 0, stream_syncs = 0, device_syncs = 0;
  int fail_alloc = 0; // n > 0: the n-th hipMalloc from now fails
};
inline StubHip g_hip;

inline const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "ok" : "out of memory (stub)"; }
inline hipError_t  hipMalloc(void** p, size_t n)
{
  if (g_hip.fail_alloc && --g_hip.fail_alloc == 0) return hipErrorOutOfMemory;
  g_hip.allocs++;
  *p = malloc(n ? n : 1);
  return hipSuccess;
}
inline hipError_t hipFree(void* p)
{
  g_hip.frees++;
  free(p);
  return hipSuccess;
}
inline hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind)
{
  g_hip.copies++;
  memcpy(d, s, n);
  return hipSuccess;
}
inline hipError_t hipStreamSynchronize(hipStream_t) { return g_hip.stream_syncs++, hipSuccess; }
inline hipError_t hipDeviceSynchronize() { return g_hip.device_syncs++, hipSuccess; }
