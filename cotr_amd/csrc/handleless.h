// Host plumbing of the entry points that take no cotr_handle (triangulate.hip, delaunay.hip, warp.hip, reproject.hip, overlap.hip,
// rotate.hip, tsdf.hip, icp.hip, structure.hip, bundle.hip, and through ransac.h guided.hip, homography.hip, essential.hip, pnp.hip,
// rigid3d.hip): a failure is reported through a per-thread message that cotr_raster_last_error() returns (handleless.hip), and the
// scratch of a call is cut into its regions by one Carver.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cotr_hip.h"

namespace cotr_detail {

// keeps msg as the calling thread's message and returns code
int handleless_fail(int code, const char* msg);

// COTR_ERR_ARG with the message "<fn>: <what><note>"
int arg_fail(const char* fn, const char* what, const char* note = "");

// after the launches of a call: the runtime's last error as the call's result
inline int launched() {
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? handleless_fail(COTR_ERR_HIP, hipGetErrorString(e)) : COTR_OK;
}

// a is a power of two (256: every region of a scratch layout starts on its own 256 bytes)
inline size_t align_up(size_t n, size_t a = 256) { return (n + a - 1) & ~(a - 1); }

inline bool aligned(const void* p, size_t a) { return (uintptr_t)p % a == 0; }

// Cuts the scratch of a call into regions that each start on their own 256 bytes, from `offset` on (the bytes of an RsPlan or
// RfPlan in front).  With a NULL base it hands out NULL and only measures, so one layout function of an op serves its
// *_scratch_bytes entry point and the call.
struct Carver {
  char* base;
  size_t bytes;   // taken so far, `offset` included
  explicit Carver(void* base, size_t offset = 0) : base(static_cast<char*>(base)), bytes(offset) {}
  template <class T>
  T* take(size_t count) {
    T* p = base ? reinterpret_cast<T*>(base + bytes) : nullptr;
    bytes += align_up(count * sizeof(T));
    return p;
  }
};

// the grid's y dimension carries the items of a call; a map's pixel count stays an int with room for the padding of a block
constexpr int MAX_ITEMS = 65535;
constexpr int MAX_PIXELS = 1 << 28;

}  // namespace cotr_detail
