// The pinhole camera of the pose and structure estimators (essential.hip, pnp.hip, structure.hip): five entries of an
// upper-triangular camera matrix, the rule that admits one, and the rule that takes a pixel to normalised coordinates.  Include only from files compiled with
// -ffp-contract=off: no product may be contracted into an FMA.
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

// y = (v - cy) / fy, then x = (u - cx - s y) / fx, of the pixel rounded to float32
ES_HD __forceinline__ void es_normalise(const EsCam& k, double u, double v, double* x, double* y) {
  u = (double)(float)u, v = (double)(float)v;
  const double yy = (v - k.cy) / k.fy;
  *x = (u - k.cx - k.s * yy) / k.fx;
  *y = yy;
}
