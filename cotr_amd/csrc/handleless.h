// Host plumbing of the entry points that take no cotr_handle (triangulate.hip, delaunay.hip, warp.hip, reproject.hip, overlap.hip,
// rotate.hip, tsdf.hip, icp.hip, icp_multi.hip, mvdepth.hip, photodepth.hip, structure.hip, bundle.hip, tracks.hip, keypoints.hip, and through ransac.h guided.hip,
// homography.hip, essential.hip, pnp.hip, rigid3d.hip): a failure is reported through a per-thread message that
// cotr_raster_last_error() returns (handleless.hip), the scratch of a call is cut into its regions by one Carver,
// and the calls that count into info_out begin with one kernel (below).
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

// The first launch of the calls that count into info_out (tsdf.hip, mvdepth.hip, photodepth.hip), one workgroup of 64: a thread per row of n <= 64
// rows of `cols` counters, column 0 = found[row] != 0 (1 without found), the rest 0.  A template (launched as hl_begin_kernel<>)
// so that only a file that launches it gets a copy: an unused static kernel would be emitted in every file that includes this.
template <int = 0>
__global__ __launch_bounds__(64) void hl_begin_kernel(const int32_t* __restrict__ found, int n, int cols, int32_t* __restrict__ info) {
  const int c = threadIdx.x;
  if (c >= n) return;
  info[c * cols] = found ? (found[c] != 0 ? 1 : 0) : 1;
  for (int i = 1; i < cols; ++i) info[c * cols + i] = 0;
}
