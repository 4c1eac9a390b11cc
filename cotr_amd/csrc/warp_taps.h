// The 8-bit bilinear tap body of OpenCV's INTER_LINEAR remap with BORDER_CONSTANT 0, shared by warp.hip
// (cotr_warp_map, cotr_warp_perspective) and rotate.hip (cotr_rotate_captures): one destination pixel from a source position
// in 1/32 px.  ix = X >> 5 (floor), fx = X & 31; taps (ix, iy), (ix+1, iy), (ix, iy+1), (ix+1, iy+1) with the integer weights
// (32-fx)(32-fy), fx(32-fy), (32-fx)fy, fx fy (sum 1024); a tap outside the source reads 0; dst = (sum w p + 512) >> 10.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

namespace cotr_detail {

// the 2 C bytes of two horizontally adjacent pixels, by loads that stay inside them
template <int C>
__device__ __forceinline__ void load_pair(const uint8_t* __restrict__ p, uint8_t* t) {
  if (C == 1) {
    uint16_t a;
    memcpy(&a, p, 2);
    t[0] = a & 255, t[1] = a >> 8;
  } else if (C == 3) {
    uint32_t a, b;
    memcpy(&a, p, 4);
    memcpy(&b, p + 2, 4);
    t[0] = a & 255, t[1] = (a >> 8) & 255, t[2] = (a >> 16) & 255;
    t[3] = (b >> 8) & 255, t[4] = (b >> 16) & 255, t[5] = b >> 24;
  } else {
    uint32_t a, b;
    memcpy(&a, p, 4);
    memcpy(&b, p + 4, 4);
    t[0] = a & 255, t[1] = (a >> 8) & 255, t[2] = (a >> 16) & 255, t[3] = a >> 24;
    t[4] = b & 255, t[5] = (b >> 8) & 255, t[6] = (b >> 16) & 255, t[7] = b >> 24;
  }
}

// one destination pixel from its fixed-point source position; returns its cover
template <int C>
__device__ __forceinline__ bool sample(const uint8_t* __restrict__ src, int Hs, int Ws, int X, int Y, uint8_t* out) {
  const int ix = X >> 5, iy = Y >> 5, fx = X & 31, fy = Y & 31;   // >> of a negative int is floor
  const int w[4] = {(32 - fx) * (32 - fy), fx * (32 - fy), (32 - fx) * fy, fx * fy};
  if (ix >= 0 && iy >= 0 && ix + 1 < Ws && iy + 1 < Hs) {        // all four taps inside
    const uint8_t* p = src + ((size_t)iy * Ws + ix) * C;
    uint8_t t[2 * C], b[2 * C];
    load_pair<C>(p, t);
    load_pair<C>(p + (size_t)Ws * C, b);
#pragma unroll
    for (int c = 0; c < C; ++c) out[c] = (uint8_t)((w[0] * t[c] + w[1] * t[C + c] + w[2] * b[c] + w[3] * b[C + c] + 512) >> 10);
    return true;
  }
  int acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0;
  bool cov = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = ix + (k & 1), y = iy + (k >> 1);
    if (x >= 0 && x < Ws && y >= 0 && y < Hs && w[k] != 0) {
      cov = true;
      const uint8_t* p = src + ((size_t)y * Ws + x) * C;
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] += w[k] * p[c];
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) out[c] = (uint8_t)((acc[c] + 512) >> 10);
  return cov;
}

}  // namespace cotr_detail
