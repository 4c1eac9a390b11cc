// The rotation augmentation of the reference's datasets: the device side of rotate_captures (cotr_amd/data.py), which
// replaces capture.rotate_capture's two cv2.warpAffine calls (image INTER_LINEAR, depth INTER_NEAREST, both about the centre
// (W/2, H/2), BORDER_CONSTANT 0).  The rule is that of OpenCV's warpAffine, stated in DESIGN.md 3l:
//   - m[0..5] maps a destination pixel to the source (the host inverts getRotationMatrix2D as warpAffine does);
//   - per destination pixel (x, y), in double and in this order of operations (no contraction), AB_BITS = 10:
//       ad = rint((m0 x) 1024), bd = rint((m3 x) 1024), X0 = rint(((m1 y) + m2) 1024), Y0 = rint(((m4 y) + m5) 1024),
//     rint = ties to even, saturated to int32;
//   - image: X = (X0 + 16 + ad) >> 5, Y alike: the position in 1/32 px, then the 8-bit bilinear of warp_taps.h;
//   - depth: X = (X0 + 512 + ad) >> 10, Y alike: dst = src[Y, X] if inside, else 0; the 32 bits are copied, not computed with.
// ONE launch for a batch of captures of any mix of shapes, images and depths together: grid.y is the item, grid.x the tiles of
// a max_h x max_w canvas (a workgroup whose tile lies outside its item's shape returns at once); a 256-thread workgroup owns a
// ROT_TW x ROT_TH tile of the destination and a lane produces ROT_PX adjacent pixels, the shape warp.hip measured as best for
// the same access pattern.  No LDS, no host waits, no allocation: capturable.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "handleless.h"
#include "warp_taps.h"

using namespace cotr_detail;

#define ROT_TW 64
#define ROT_TH 16
#define ROT_PX 4               // adjacent pixels per lane
#define ROT_THREADS (ROT_TW / ROT_PX * ROT_TH)
#define ROT_MAX 16384
static_assert(ROT_PX == 4 && ROT_TW % ROT_PX == 0 && ROT_THREADS % 64 == 0 && ROT_THREADS <= 1024, "tile shape");

// saturate_cast<int>(rint(v)); a NaN goes to INT_MIN
__device__ __forceinline__ int rint_sat(double v) { return (int)rint(fmin(fmax(v, (double)INT_MIN), (double)INT_MAX)); }

// a + b + c as int32 that wraps (a rotation of a side <= 16384 stays below 2^27; a foreign matrix must not be undefined)
__device__ __forceinline__ int add3(int a, int b, int c) { return (int)((unsigned)a + (unsigned)b + (unsigned)c); }

__global__ __launch_bounds__(ROT_THREADS) void rotate_kernel(const unsigned long long* __restrict__ ptrs,
                                                             const int32_t* __restrict__ shapes, const double* __restrict__ mats,
                                                             int tiles_x) {
  const int item = blockIdx.y;
  const int H = shapes[2 * item], W = shapes[2 * item + 1];
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x % tiles_x;
  if (H < 1 || W < 1 || H > ROT_MAX || W > ROT_MAX || ty * ROT_TH >= H || tx * ROT_TW >= W) return;   // the whole workgroup
  const int i = ty * ROT_TH + threadIdx.x / (ROT_TW / ROT_PX);
  const int j0 = tx * ROT_TW + threadIdx.x % (ROT_TW / ROT_PX) * ROT_PX;
  if (i >= H || j0 >= W) return;
  const uint8_t* __restrict__ isrc = reinterpret_cast<const uint8_t*>(ptrs[4 * item]);
  uint8_t* __restrict__ idst = reinterpret_cast<uint8_t*>(ptrs[4 * item + 1]);
  const uint32_t* __restrict__ dsrc = reinterpret_cast<const uint32_t*>(ptrs[4 * item + 2]);
  uint32_t* __restrict__ ddst = reinterpret_cast<uint32_t*>(ptrs[4 * item + 3]);
  const double* __restrict__ m = mats + 6 * (size_t)item;
  const int n = min(ROT_PX, W - j0);
  const size_t p = (size_t)i * W + j0;

  // X0 + ad, Y0 + bd: once per pixel, for both halves
  const double y = (double)i;
  const int X0 = rint_sat(((m[1] * y) + m[2]) * 1024.0), Y0 = rint_sat(((m[4] * y) + m[5]) * 1024.0);
  int ad[ROT_PX], bd[ROT_PX];
#pragma unroll
  for (int k = 0; k < ROT_PX; ++k) {
    const double x = (double)(j0 + k);
    ad[k] = rint_sat((m[0] * x) * 1024.0), bd[k] = rint_sat((m[3] * x) * 1024.0);
  }

  if (isrc && idst) {
    uint8_t o[ROT_PX * 3];
#pragma unroll
    for (int k = 0; k < ROT_PX; ++k)
      if (k < n) sample<3>(isrc, H, W, add3(X0, 16, ad[k]) >> 5, add3(Y0, 16, bd[k]) >> 5, o + k * 3);
    uint8_t* d = idst + p * 3;
    if (n == ROT_PX && ((uintptr_t)d & 3) == 0) {
      uint32_t w[3];
      memcpy(w, o, 12);
#pragma unroll
      for (int c = 0; c < 3; ++c) reinterpret_cast<uint32_t*>(d)[c] = w[c];
    } else {
#pragma unroll
      for (int k = 0; k < ROT_PX; ++k)
        if (k < n) {
#pragma unroll
          for (int c = 0; c < 3; ++c) d[k * 3 + c] = o[k * 3 + c];
        }
    }
  }

  if (dsrc && ddst) {
    uint32_t v[ROT_PX];
#pragma unroll
    for (int k = 0; k < ROT_PX; ++k) {
      const int X = add3(X0, 512, ad[k]) >> 10, Y = add3(Y0, 512, bd[k]) >> 10;   // >> of a negative int is floor
      v[k] = (k < n && X >= 0 && X < W && Y >= 0 && Y < H) ? dsrc[(size_t)Y * W + X] : 0u;
    }
    uint32_t* d = ddst + p;
    if (n == ROT_PX && ((uintptr_t)d & 15) == 0) {
      *reinterpret_cast<uint4*>(d) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int k = 0; k < ROT_PX; ++k)
        if (k < n) d[k] = v[k];
    }
  }
}

extern "C" {

int cotr_rotate_captures(const uint64_t* ptrs, const int32_t* shapes, const double* mats, int n, int max_h, int max_w,
                         cotr_stream stream) {
  if (!ptrs || !shapes || !mats) return handleless_fail(COTR_ERR_ARG, "ptrs, shapes and mats must not be NULL");
  if (n < 1 || n > MAX_ITEMS) return handleless_fail(COTR_ERR_ARG, "n must be in [1, 65535]");
  if (max_h < 1 || max_h > ROT_MAX || max_w < 1 || max_w > ROT_MAX)
    return handleless_fail(COTR_ERR_ARG, "max_h and max_w must be in [1, 16384]");
  if (!aligned(ptrs, 8) || !aligned(mats, 8) || !aligned(shapes, 4))
    return handleless_fail(COTR_ERR_ARG, "ptrs and mats must be 8-byte, shapes 4-byte aligned");
  const int tiles_x = (max_w + ROT_TW - 1) / ROT_TW, tiles_y = (max_h + ROT_TH - 1) / ROT_TH;   // at most 256 x 1024
  hipLaunchKernelGGL(rotate_kernel, dim3(tiles_x * tiles_y, n), dim3(ROT_THREADS), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const unsigned long long*>(ptrs), shapes, mats, tiles_x);
  return launched();
}

}  // extern "C"
