// The pixel rule of the vertex and normal maps (icp.hip: cotr_icp_depth, icp_multi.hip: cotr_icp_maps), stated once.  Rules in
// DESIGN.md 3h-9; the vertex is pinhole.h's.  Included by translation units compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "pinhole.h"

// Pixel (x, y) of a H x W map -> its vertex v (es_vertex) and its normal n, NaN where there is none; true when it has a normal: an
// interior pixel whose five depths are valid, whose four neighbours lie within edge z of its depth, and whose central
// differences have a cross product that is not 0.  The normal is turned towards the camera.
__device__ __forceinline__ bool ic_pixel(const float* __restrict__ depth, int H, int W, const EsCam& k, double edge, int x, int y, double* v,
                                         double* n) {
  n[0] = n[1] = n[2] = NAN;
  bool ok = es_vertex(depth, W, k, x, y, v);
  if (!ok) v[0] = v[1] = v[2] = NAN;
  if (ok && x > 0 && x < W - 1 && y > 0 && y < H - 1) {
    double l[3], r[3], u[3], d[3];
    ok = es_vertex(depth, W, k, x - 1, y, l) && es_vertex(depth, W, k, x + 1, y, r) && es_vertex(depth, W, k, x, y - 1, u) &&
         es_vertex(depth, W, k, x, y + 1, d);
    if (ok) {
      const double lim = edge * v[2];
      ok = fabs(l[2] - v[2]) <= lim && fabs(r[2] - v[2]) <= lim && fabs(u[2] - v[2]) <= lim && fabs(d[2] - v[2]) <= lim;
    }
    if (ok) {
      const double ax = r[0] - l[0], ay = r[1] - l[1], az = r[2] - l[2];
      const double bx = d[0] - u[0], by = d[1] - u[1], bz = d[2] - u[2];
      const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
      const double norm = sqrt((cx * cx + cy * cy) + cz * cz);
      ok = norm > 0.0;   // false for NaN
      if (ok) {
        n[0] = cx / norm, n[1] = cy / norm, n[2] = cz / norm;
        if ((n[0] * v[0] + n[1] * v[1]) + n[2] * v[2] > 0.0) n[0] = -n[0], n[1] = -n[1], n[2] = -n[2];
      }
    }
  } else {
    ok = false;
  }
  return ok;
}
