// Host plumbing of the entry points that take no cotr_handle (triangulate.hip, guided.hip, warp.hip, reproject.hip,
// overlap.hip, rotate.hip): they report a failure through a per-thread message that cotr_raster_last_error() returns (handleless.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cotr_hip.h"

namespace cotr_detail {

// keeps msg as the calling thread's message and returns code
int handleless_fail(int code, const char* msg);

// after the launches of a call: the runtime's last error as the call's result
inline int launched() {
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? handleless_fail(COTR_ERR_HIP, hipGetErrorString(e)) : COTR_OK;
}

// a is a power of two (256: every region of a scratch layout starts on its own 256 bytes)
inline size_t align_up(size_t n, size_t a = 256) { return (n + a - 1) & ~(a - 1); }

inline bool aligned(const void* p, size_t a) { return (uintptr_t)p % a == 0; }

// the grid's y dimension carries the items of a call; a map's pixel count stays an int with room for the padding of a block
constexpr int MAX_ITEMS = 65535;
constexpr int MAX_PIXELS = 1 << 28;

}  // namespace cotr_detail
