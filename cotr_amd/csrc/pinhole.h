// The pinhole camera of the pose and structure estimators and of the depth-map ops (essential.hip, pnp.hip, structure.hip, icp.hip,
// icp_multi.hip, tsdf.hip, mvdepth.hip), stated once: five entries of an upper-triangular camera matrix and the rule that admits one,
// pixel <-> normalised coordinates, the nearest pixel of a map, the vertex of a depth map's pixel, the row-major 4 x 4 pose applied to
// a point and its rigid inverse, and the cameras of a call.  Include only from files compiled with -ffp-contract=off.
#pragma once
#include <math.h>

#define ES_HD __host__ __device__

// fx, fy, cx, cy, skew of an upper-triangular camera matrix
struct EsCam {
  double fx, fy, cx, cy, s;
};

// the camera of an upper-triangular K (row-major 9 doubles, on the host); false unless fx and fy are finite and non-zero and
// the rest is finite
inline bool es_camera(const double* K, EsCam* c) {
  c->fx = K[0], c->s = K[1], c->cx = K[2], c->fy = K[4], c->cy = K[5];
  const bool finite = isfinite(c->fx) && isfinite(c->fy) && isfinite(c->cx) && isfinite(c->cy) && isfinite(c->s);
  return finite && c->fx != 0.0 && c->fy != 0.0;
}

// y = (v - cy) / fy, then x = (u - cx - s y) / fx, of the pixel as it is
ES_HD __forceinline__ void es_ray(const EsCam& k, double u, double v, double* x, double* y) {
  const double yy = (v - k.cy) / k.fy;
  *x = (u - k.cx - k.s * yy) / k.fx;
  *y = yy;
}

// es_ray of the pixel rounded to float32
ES_HD __forceinline__ void es_normalise(const EsCam& k, double u, double v, double* x, double* y) { es_ray(k, (double)(float)u, (double)(float)v, x, y); }

// camera point Y -> pixel, not rounded: u = (fx xn + s yn) + cx, v = fy yn + cy of (xn, yn) = (Y_x, Y_y) / Y_z; false unless Y_z > 0 (NaN too)
ES_HD __forceinline__ bool es_project(const EsCam& k, const double* Y, double* u, double* v) {
  if (!(Y[2] > 0.0)) return false;
  const double xn = Y[0] / Y[2], yn = Y[1] / Y[2];
  *u = (k.fx * xn + k.s * yn) + k.cx, *v = k.fy * yn + k.cy;
  return true;
}

// the pixel (*x, *y) of an H x W map nearest (u, v), ties to even (row-major index (size_t)y W + x); false outside the map, NaN too
ES_HD __forceinline__ bool es_nearest(double u, double v, int H, int W, int* x, int* y) {
  const double ru = rint(u), rv = rint(v);
  if (!(ru >= 0.0 && ru < (double)W && rv >= 0.0 && rv < (double)H)) return false;
  *x = (int)ru, *y = (int)rv;
  return true;
}

// the vertex of the pixel centre (x, y) of a depth map with rows of W: (xn z, yn z, z); false where the depth is not finite and > 0
__device__ __forceinline__ bool es_vertex(const float* __restrict__ depth, int W, const EsCam& k, int x, int y, double* v) {
  const double z = (double)depth[(size_t)y * W + x];
  if (!(z > 0.0 && z < INFINITY)) return false;
  double xn, yn;
  es_ray(k, (double)x, (double)y, &xn, &yn);
  v[0] = xn * z, v[1] = yn * z, v[2] = z;
  return true;
}

// ---- the pose m: row-major 4 x 4 [R | t], camera-to-world; o = R d, and o = R^T d -----------------------------------------------
ES_HD __forceinline__ void es_rotate(const double* m, const double* d, double* o) {
  for (int a = 0; a < 3; ++a) o[a] = (m[a * 4] * d[0] + m[a * 4 + 1] * d[1]) + m[a * 4 + 2] * d[2];
}
ES_HD __forceinline__ void es_unrotate(const double* m, const double* d, double* o) {
  for (int a = 0; a < 3; ++a) o[a] = (m[a] * d[0] + m[4 + a] * d[1]) + m[8 + a] * d[2];
}

// camera point Y -> world: R Y + t
ES_HD __forceinline__ void es_to_world(const double* m, const double* Y, double* P) {
  es_rotate(m, Y, P);
  P[0] = P[0] + m[3], P[1] = P[1] + m[7], P[2] = P[2] + m[11];
}

// world point P -> camera, the rigid inverse: R^T (P - t)
ES_HD __forceinline__ void es_to_camera(const double* m, const double* P, double* Y) {
  const double d[3] = {P[0] - m[3], P[1] - m[7], P[2] - m[11]};
  es_unrotate(m, d, Y);
}

// ---- the cameras of a call: a kernel argument, read at a uniform index --------------------------------------------------------
#define ES_MAX_CAMS 32
struct EsCams {
  EsCam k[ES_MAX_CAMS];
};
static const char* const ES_CAMERAS_WHAT = "the camera matrices must be finite with focal lengths that are not 0";

// Ks [n][9] -> the first n rows of cams, the rest {1, 1, 0, 0, 0}; ES_CAMERAS_WHAT at the first row es_camera refuses, else NULL
inline const char* es_cameras(const double* Ks, int n, EsCams* cams) {
  for (int c = 0; c < ES_MAX_CAMS; ++c) cams->k[c] = EsCam{1.0, 1.0, 0.0, 0.0, 0.0};
  for (int c = 0; c < n; ++c)
    if (!es_camera(Ks + c * 9, &cams->k[c])) return ES_CAMERAS_WHAT;
  return nullptr;
}
