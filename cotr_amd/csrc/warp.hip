// Bilinear warps of 8-bit images: the device side of warp_by_map / warp_perspective (cotr_amd/inference/warp.py), which
// replace the cv2.remap of demo_single_pair.py:43 and the cv2.warpPerspective pair + composite of demo_homography.py:46-49.
// The rule is that of OpenCV's 8-bit INTER_LINEAR remap with BORDER_CONSTANT 0, stated in DESIGN.md 3i:
//   - coordinates are pixel indices (sample (j, i) is the centre of src[i, j]), fixed to 1/32 px: X = rint(v * 32), ties to
//     even, v the float32 map value (a float64 map is rounded to float32 first); ix = X >> 5 (floor), fx = X & 31;
//     a non-finite v or |v| >= 2^26 puts all four taps outside;
//   - taps (ix, iy), (ix+1, iy), (ix, iy+1), (ix+1, iy+1) with the integer weights (32-fx)(32-fy), fx(32-fy), (32-fx)fy,
//     fx fy (sum 1024); a tap outside the source reads 0; dst = (sum w p + 512) >> 10;
//   - cover = 1 where a tap with a non-zero weight lies inside the source; with a background, an uncovered pixel takes the
//     background's pixel instead of the border value;
//   - perspective: per destination pixel (x, y), in double and in this order of operations (no contraction),
//     W = (m6 x + m7 y) + m8, W = W != 0 ? 32 / W : 0, X = rint(clamp(((m0 x + m1 y) + m2) W, INT_MIN, INT_MAX)), Y alike;
//     W == 0 or a NaN coordinate puts all four taps outside.
// One launch per call: a 256-thread workgroup owns a WARP_TW x WARP_TH tile of the destination (its taps fall into a compact
// patch of the source), a lane produces WARP_PX adjacent pixels and writes them as whole dwords where the row allows it.
// No host waits, no allocation: capturable.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "handleless.h"
#include "warp_taps.h"   // load_pair, sample: the tap body, shared with rotate.hip

using namespace cotr_detail;

#ifndef WARP_TW
#define WARP_TW 64             // tile width and height in destination pixels (what was tried)
#endif
#ifndef WARP_TH
#define WARP_TH 16
#endif
#define WARP_PX 4              // adjacent pixels per lane
#define WARP_THREADS (WARP_TW / WARP_PX * WARP_TH)
#define WARP_MAX 16384
#define WARP_OUTSIDE INT_MIN   // a fixed-point coordinate whose taps (ix = -2^26, ix + 1) are outside every source
static_assert(WARP_TW % WARP_PX == 0 && WARP_THREADS % 64 == 0 && WARP_THREADS <= 1024, "tile shape");

struct WarpM {
  double m[9];
};

__device__ __forceinline__ int fix_f32(float v) {
  return fabsf(v) < 67108864.f ? (int)rintf(v * 32.f) : WARP_OUTSIDE;   // false for NaN and inf; v * 32 is exact
}

__device__ __forceinline__ int fix_f64(double v) {
  if (v != v) return WARP_OUTSIDE;
  return (int)rint(fmin(fmax(v, (double)INT_MIN), (double)INT_MAX));
}

struct MapCoords {
  const void* map;
  int is_f64;
  // (X, Y) of the n <= WARP_PX pixels from p = i * Wd + j0 on; the others are left alone
  __device__ __forceinline__ void get(size_t p, int, int, int n, int* X, int* Y) const {
    if (is_f64) {
      const double2* m = static_cast<const double2*>(map) + p;
#pragma unroll
      for (int k = 0; k < WARP_PX; ++k)
        if (k < n) {
          const double2 v = m[k];
          X[k] = fix_f32((float)v.x), Y[k] = fix_f32((float)v.y);
        }
    } else {
      const float2* m = static_cast<const float2*>(map) + p;
      if (n == WARP_PX && ((uintptr_t)m & 15) == 0) {
        static_assert(WARP_PX == 4, "two float4 per lane");
        const float4 a = reinterpret_cast<const float4*>(m)[0], b = reinterpret_cast<const float4*>(m)[1];
        X[0] = fix_f32(a.x), Y[0] = fix_f32(a.y), X[1] = fix_f32(a.z), Y[1] = fix_f32(a.w);
        X[2] = fix_f32(b.x), Y[2] = fix_f32(b.y), X[3] = fix_f32(b.z), Y[3] = fix_f32(b.w);
      } else {
#pragma unroll
        for (int k = 0; k < WARP_PX; ++k)
          if (k < n) {
            const float2 v = m[k];
            X[k] = fix_f32(v.x), Y[k] = fix_f32(v.y);
          }
      }
    }
  }
};

struct PerspCoords {
  WarpM M;
  __device__ __forceinline__ void get(size_t, int i, int j0, int n, int* X, int* Y) const {
    const double y = (double)i;
#pragma unroll
    for (int k = 0; k < WARP_PX; ++k)
      if (k < n) {
        const double x = (double)(j0 + k);
        double W = (M.m[6] * x + M.m[7] * y) + M.m[8];
        const bool horizon = W == 0.0;
        W = horizon ? 0.0 : 32.0 / W;
        const double fx = ((M.m[0] * x + M.m[1] * y) + M.m[2]) * W;
        const double fy = ((M.m[3] * x + M.m[4] * y) + M.m[5]) * W;
        X[k] = horizon ? WARP_OUTSIDE : fix_f64(fx);
        Y[k] = horizon ? WARP_OUTSIDE : fix_f64(fy);
      }
  }
};

// WARP_PX pixels of C bytes at p: whole dwords (one 16-byte access for C == 4) where p allows it
template <int C>
__device__ __forceinline__ void store_group(uint8_t* p, const uint8_t* o) {
  uint32_t w[C];
  memcpy(w, o, 4 * C);
  if (C == 4 && ((uintptr_t)p & 15) == 0) {
    *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) reinterpret_cast<uint32_t*>(p)[c] = w[c];
  }
}

template <int C>
__device__ __forceinline__ void load_group(const uint8_t* p, uint8_t* o) {
  uint32_t w[C];
  if (C == 4 && ((uintptr_t)p & 15) == 0) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) w[c] = reinterpret_cast<const uint32_t*>(p)[c];
  }
  memcpy(o, w, 4 * C);
}

template <int C, class Coords>
__device__ __forceinline__ void warp_lane(const Coords& coords, const uint8_t* __restrict__ src, int Hs, int Ws, int Hd, int Wd,
                                          uint8_t* __restrict__ dst, uint8_t* __restrict__ cover,
                                          const uint8_t* __restrict__ background) {
  const int i = blockIdx.y * WARP_TH + threadIdx.x / (WARP_TW / WARP_PX);
  const int j0 = blockIdx.x * WARP_TW + threadIdx.x % (WARP_TW / WARP_PX) * WARP_PX;
  if (i >= Hd || j0 >= Wd) return;
  const int n = min(WARP_PX, Wd - j0);
  const size_t p = (size_t)i * Wd + j0;
  int X[WARP_PX], Y[WARP_PX];
  coords.get(p, i, j0, n, X, Y);
  uint8_t o[WARP_PX * C];
  bool cv[WARP_PX];
  bool all = true;
#pragma unroll
  for (int k = 0; k < WARP_PX; ++k) {
    cv[k] = k < n && sample<C>(src, Hs, Ws, X[k], Y[k], o + k * C);
    all = all && cv[k];
  }
  uint8_t* d = dst + p * C;
  const uint8_t* g = background ? background + p * C : nullptr;
  if (n == WARP_PX && ((uintptr_t)d & 3) == 0 && ((uintptr_t)g & 3) == 0) {
    if (g && !all) {
      uint8_t b[WARP_PX * C];
      load_group<C>(g, b);
#pragma unroll
      for (int k = 0; k < WARP_PX; ++k)
#pragma unroll
        for (int c = 0; c < C; ++c) o[k * C + c] = cv[k] ? o[k * C + c] : b[k * C + c];
    }
    store_group<C>(d, o);
  } else {
#pragma unroll
    for (int k = 0; k < WARP_PX; ++k)
      if (k < n) {
#pragma unroll
        for (int c = 0; c < C; ++c) d[k * C + c] = (g && !cv[k]) ? g[k * C + c] : o[k * C + c];
      }
  }
  if (cover) {
    if (n == WARP_PX && ((uintptr_t)(cover + p) & 3) == 0) {
      *reinterpret_cast<uint32_t*>(cover + p) =
          (uint32_t)cv[0] | (uint32_t)cv[1] << 8 | (uint32_t)cv[2] << 16 | (uint32_t)cv[3] << 24;
    } else {
#pragma unroll
      for (int k = 0; k < WARP_PX; ++k)
        if (k < n) cover[p + k] = cv[k];
    }
  }
}

template <class Coords>
__device__ __forceinline__ void warp_any_c(const Coords& coords, const uint8_t* src, int Hs, int Ws, int C, int Hd, int Wd,
                                           uint8_t* dst, uint8_t* cover, const uint8_t* background) {
  if (C == 3) warp_lane<3>(coords, src, Hs, Ws, Hd, Wd, dst, cover, background);        // (C is the same in every lane)
  else if (C == 1) warp_lane<1>(coords, src, Hs, Ws, Hd, Wd, dst, cover, background);
  else warp_lane<4>(coords, src, Hs, Ws, Hd, Wd, dst, cover, background);
}

__global__ __launch_bounds__(WARP_THREADS) void warp_map_kernel(const uint8_t* __restrict__ src, int Hs, int Ws, int C,
                                                                const void* __restrict__ map, int map_is_f64, int Hd, int Wd,
                                                                uint8_t* __restrict__ dst, uint8_t* __restrict__ cover,
                                                                const uint8_t* __restrict__ background) {
  warp_any_c(MapCoords{map, map_is_f64}, src, Hs, Ws, C, Hd, Wd, dst, cover, background);
}

__global__ __launch_bounds__(WARP_THREADS) void warp_perspective_kernel(const uint8_t* __restrict__ src, int Hs, int Ws, int C,
                                                                        WarpM M, int Hd, int Wd, uint8_t* __restrict__ dst,
                                                                        uint8_t* __restrict__ cover,
                                                                        const uint8_t* __restrict__ background) {
  warp_any_c(PerspCoords{M}, src, Hs, Ws, C, Hd, Wd, dst, cover, background);
}

// ---- host side ------------------------------------------------------------------------------------------------------
namespace {

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

const char* warp_check(const uint8_t* src, int Hs, int Ws, int C, int Hd, int Wd, const uint8_t* dst, const uint8_t* background) {
  if (C != 1 && C != 3 && C != 4) return "C must be 1, 3 or 4";
  if (Hs < 1 || Hs > WARP_MAX || Ws < 1 || Ws > WARP_MAX || Hd < 1 || Hd > WARP_MAX || Wd < 1 || Wd > WARP_MAX)
    return "source and destination H and W must be in [1, 16384]";
  if (!src || !dst) return "src and dst must not be NULL";
  const size_t nd = (size_t)Hd * Wd * C;
  if (overlap(dst, nd, src, (size_t)Hs * Ws * C)) return "dst must not alias src";
  if (background && overlap(dst, nd, background, nd)) return "dst must not alias background";
  return nullptr;
}

dim3 warp_grid(int Hd, int Wd) { return dim3((Wd + WARP_TW - 1) / WARP_TW, (Hd + WARP_TH - 1) / WARP_TH); }

}  // namespace

extern "C" {

int cotr_warp_map(const uint8_t* src, int Hs, int Ws, int C, const void* map, int map_is_f64, int Hd, int Wd, uint8_t* dst,
                  uint8_t* cover, const uint8_t* background, cotr_stream stream) {
  if (const char* e = warp_check(src, Hs, Ws, C, Hd, Wd, dst, background)) return handleless_fail(COTR_ERR_ARG, e);
  if (!map) return handleless_fail(COTR_ERR_ARG, "map must not be NULL");
  if (!aligned(map, map_is_f64 ? 16 : 8))
    return handleless_fail(COTR_ERR_ARG, "a float32 map must be 8-byte and a float64 map 16-byte aligned");
  hipLaunchKernelGGL(warp_map_kernel, warp_grid(Hd, Wd), dim3(WARP_THREADS), 0, static_cast<hipStream_t>(stream), src, Hs, Ws, C,
                     map, map_is_f64 ? 1 : 0, Hd, Wd, dst, cover, background);
  return launched();
}

int cotr_warp_perspective(const uint8_t* src, int Hs, int Ws, int C, const double* M, int Hd, int Wd, uint8_t* dst,
                          uint8_t* cover, const uint8_t* background, cotr_stream stream) {
  if (const char* e = warp_check(src, Hs, Ws, C, Hd, Wd, dst, background)) return handleless_fail(COTR_ERR_ARG, e);
  if (!M) return handleless_fail(COTR_ERR_ARG, "M must not be NULL");
  WarpM m;
  for (int k = 0; k < 9; ++k) {
    if (!(fabs(M[k]) < INFINITY)) return handleless_fail(COTR_ERR_ARG, "M must be finite");
    m.m[k] = M[k];
  }
  hipLaunchKernelGGL(warp_perspective_kernel, warp_grid(Hd, Wd), dim3(WARP_THREADS), 0, static_cast<hipStream_t>(stream), src, Hs,
                     Ws, C, m, Hd, Wd, dst, cover, background);
  return launched();
}

}  // extern "C"
