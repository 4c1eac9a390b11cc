// The camera rule of reproject.hip and overlap.hip, everything in double, products and sums in this order.
// Include only from files compiled with -ffp-contract=off: no product may be contracted into an FMA.
//   pixel (x, y) with depth z -> camera point -> world point (pixel_to_world):
//     c = (Kinv . (x, y, 1)) * z, a row being (k0 x + k1 y) + k2          reject unless z > 0 and c.z > 0
//     w = c2w . (c, 1), a row being ((m0 c.x + m1 c.y) + m2 c.z) + m3      reject if w.w == 0, then w.xyz /= w.w
//   world point X -> pixel of a camera with the 3x4 projection P (project_inside):
//     p = P . (X, 1), rows as above                                        reject unless p.z > 0
//     u = p.x / p.z, v = p.y / p.z                                         reject unless 0 <= u < W - 1 and 0 <= v < H - 1
#pragma once

__device__ __forceinline__ double row3(const double* __restrict__ r, double x, double y) { return (r[0] * x + r[1] * y) + r[2]; }

__device__ __forceinline__ double row4(const double* __restrict__ r, double x, double y, double z) {
  return ((r[0] * x + r[1] * y) + r[2] * z) + r[3];
}

// Kinv[9], c2w[16] row-major; w is written only when the pixel is valid
__device__ __forceinline__ bool pixel_to_world(const double* __restrict__ Kinv, const double* __restrict__ c2w, double x, double y,
                                               double z, double w[3]) {
  if (!(z > 0.0)) return false;
  const double c0 = row3(Kinv, x, y) * z, c1 = row3(Kinv + 3, x, y) * z, c2 = row3(Kinv + 6, x, y) * z;
  if (!(c2 > 0.0)) return false;
  const double w3 = row4(c2w + 12, c0, c1, c2);
  if (w3 == 0.0) return false;
  w[0] = row4(c2w, c0, c1, c2) / w3;
  w[1] = row4(c2w + 4, c0, c1, c2) / w3;
  w[2] = row4(c2w + 8, c0, c1, c2) / w3;
  return true;
}

// P[12] row-major; pz = p.z, u and v are written once pz > 0
__device__ __forceinline__ bool project_inside(const double* __restrict__ P, const double X[3], int W, int H, double& u, double& v,
                                               double& pz) {
  pz = row4(P + 8, X[0], X[1], X[2]);
  if (!(pz > 0.0)) return false;
  u = row4(P, X[0], X[1], X[2]) / pz;
  v = row4(P + 4, X[0], X[1], X[2]) / pz;
  return u >= 0.0 && u < (double)(W - 1) && v >= 0.0 && v < (double)(H - 1);   // false for NaN
}
