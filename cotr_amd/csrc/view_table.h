// The view table of the structure estimators (structure.hip: triangulation with known cameras, bundle.hip: bundle adjustment)
// and the arithmetic they share with mvdepth.hip and photodepth.hip: a view's validity, a point's pixel, a pixel's ray, the projection of a world
// point and the symmetric 3 x 3 solve by cofactors.  Rules in DESIGN.md 3h-6.  Include only from files compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pinhole.h"

#define TV_MAX_VIEWS 32
// a row of the view table: fx fy cx cy skew | R (9, row-major) | t (3) | c (3) | valid (1.0 or 0.0) | 3 unused
#define TV_ROW 24
#define TV_R 5
#define TV_T 14
#define TV_C 17
#define TV_OK 20

// ---- per-view arithmetic (w: the view's row of the table) -----------------------------------------------------------------
struct TvPixel {
  double u, v;   // rounded to float32
  bool finite;
};

__device__ __forceinline__ TvPixel tv_pixel(const double* __restrict__ points, size_t N, int v, size_t p) {
  const double2 q = *reinterpret_cast<const double2*>(points + ((size_t)v * N + p) * 2);
  const float uf = (float)q.x, vf = (float)q.y;
  return {(double)uf, (double)vf, isfinite(uf) && isfinite(vf)};
}

// the ray of pixel (u, v) through the view's centre, in the world and not normalised: R^T (xn, yn, 1), (xn, yn) by es_normalise
__device__ __forceinline__ void tv_view_ray(const double* w, double u, double v, double* r) {
  const EsCam k = {w[0], w[1], w[2], w[3], w[4]};
  double x, y;
  es_normalise(k, u, v, &x, &y);
  const double* R = w + TV_R;
  r[0] = (R[0] * x + R[3] * y) + R[6], r[1] = (R[1] * x + R[4] * y) + R[7], r[2] = (R[2] * x + R[5] * y) + R[8];
}

// Cofactors c (00 01 02 11 12 22) of the symmetric 3 x 3 matrix m (00 01 02 11 12 22); returns its determinant.
__device__ __forceinline__ double tv_cofactors(const double* m, double* c) {
  c[0] = m[3] * m[5] - m[4] * m[4], c[1] = m[2] * m[4] - m[1] * m[5], c[2] = m[1] * m[4] - m[2] * m[3];
  c[3] = m[0] * m[5] - m[2] * m[2], c[4] = m[1] * m[2] - m[0] * m[4], c[5] = m[0] * m[3] - m[1] * m[1];
  return (m[0] * c[0] + m[1] * c[1]) + m[2] * c[2];
}

// The symmetric 3 x 3 system m (00 01 02 11 12 22) x = b by cofactors, branch-free up to the verdict: false when the
// determinant is 0 or not finite, or a coordinate is not finite.
__device__ __forceinline__ bool tv_solve(const double* m, const double* b, double* x) {
  double c[6];
  const double det = tv_cofactors(m, c);
  x[0] = ((c[0] * b[0] + c[1] * b[1]) + c[2] * b[2]) / det;
  x[1] = ((c[1] * b[0] + c[3] * b[1]) + c[4] * b[2]) / det;
  x[2] = ((c[2] * b[0] + c[4] * b[1]) + c[5] * b[2]) / det;
  return det != 0.0 && isfinite(det) && isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]);
}

// X in the view: depth z, normalised (xn, yn), squared pixel distance e to the observation, residual (du, dv)
struct TvProj {
  double z, xn, yn, du, dv, e;
};

__device__ __forceinline__ TvProj tv_project(const double* w, const TvPixel& q, const double* X) {
  const double* R = w + TV_R;
  const double* t = w + TV_T;
  TvProj r;
  const double p0 = ((R[0] * X[0] + R[1] * X[1]) + R[2] * X[2]) + t[0];
  const double p1 = ((R[3] * X[0] + R[4] * X[1]) + R[5] * X[2]) + t[1];
  r.z = ((R[6] * X[0] + R[7] * X[1]) + R[8] * X[2]) + t[2];
  r.xn = p0 / r.z, r.yn = p1 / r.z;
  r.du = ((w[0] * r.xn + w[4] * r.yn) + w[2]) - q.u;
  r.dv = (w[1] * r.yn + w[3]) - q.v;
  r.e = r.du * r.du + r.dv * r.dv;
  return r;
}

// ---- the table itself ----------------------------------------------------------------------------------------------------------
// Row v of the table (the Prepare rule of DESIGN.md 3h-6): camera, pose, centre c = -R^T t and the view's validity -> w.  The one
// statement of the rule: tv_prepare_kernel writes the rows to global memory, mvdepth.hip and photodepth.hip build them in LDS.
__device__ __forceinline__ void tv_view_row(const double* __restrict__ cams, const double* __restrict__ poses, int v, double* w) {
  const double* k = cams + v * 5;
  const double* P = poses + v * 12;
  bool ok = true;
  for (int i = 0; i < 5; ++i) {
    w[i] = k[i];
    ok = ok && isfinite(k[i]);
  }
  ok = ok && k[0] != 0.0 && k[1] != 0.0;
  double t[3];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) {
      w[TV_R + r * 3 + c] = P[r * 4 + c];
      ok = ok && isfinite(P[r * 4 + c]);
    }
    t[r] = P[r * 4 + 3];
    w[TV_T + r] = t[r];
    ok = ok && isfinite(t[r]);
  }
  for (int c = 0; c < 3; ++c) {
    const double cc = -((P[c] * t[0] + P[4 + c] * t[1]) + P[8 + c] * t[2]);
    w[TV_C + c] = cc;
    ok = ok && isfinite(cc);
  }
  w[TV_OK] = ok ? 1.0 : 0.0;
  w[21] = w[22] = w[23] = 0.0;
}

// A thread per view: its row -> tab; info[0] = found, info[1..7] = 0.  One workgroup of 64 threads.  File-local (static) on purpose:
// every translation unit that includes this header gets its own copy, which is what lets the kernel live here, launched by structure.hip
// and bundle.hip alike, while structure.hip keeps the instructions it had when the kernel was defined there.  A translation unit that
// keeps no table in global memory (mvdepth.hip, photodepth.hip) defines TV_NO_PREPARE_KERNEL before the include and gets no copy.
#ifndef TV_NO_PREPARE_KERNEL
static __global__ __launch_bounds__(64) void tv_prepare_kernel(const double* __restrict__ cams, const double* __restrict__ poses, int V,
                                                        const int32_t* __restrict__ found, double* __restrict__ tab,
                                                        int32_t* __restrict__ info) {
  const int v = threadIdx.x;
  if (v < 8) info[v] = v == 0 ? (found ? (found[0] != 0) : 1) : 0;
  if (v >= V) return;
  tv_view_row(cams, poses, v, tab + v * TV_ROW);
}
#endif
