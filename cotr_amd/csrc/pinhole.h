// The pinhole camera of the pose and structure estimators (essential.hip, structure.hip): five entries of an upper-triangular
// camera matrix and the rule that takes a pixel to normalised coordinates.  Include only from files compiled with
// -ffp-contract=off: no product may be contracted into an FMA.
#pragma once

#define ES_HD __host__ __device__

// fx, fy, cx, cy, skew of an upper-triangular camera matrix
struct EsCam {
  double fx, fy, cx, cy, s;
};

// y = (v - cy) / fy, then x = (u - cx - s y) / fx, of the pixel rounded to float32
ES_HD __forceinline__ void es_normalise(const EsCam& k, double u, double v, double* x, double* y) {
  u = (double)(float)u, v = (double)(float)v;
  const double yy = (v - k.cy) / k.fy;
  *x = (u - k.cx - k.s * yy) / k.fx;
  *y = yy;
}
