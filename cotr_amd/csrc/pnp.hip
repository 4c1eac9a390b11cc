// Absolute pose from 3D-2D correspondences: P3P RANSAC with a Gauss-Newton refit on the inliers, in the structure of
// OpenCV's solvePnPRansac(SOLVEPNP_P3P), and the lift of pixels of a depth map to 3D points that feeds it.
// Rules in DESIGN.md 3h-4.  x_cam = R X + t.
//
// cotr_lift_pixels: 1 launch, one thread per point.
// cotr_ransac_pnp: 4 + 2 * (refine_iters + 1) launches on the caller's stream (4 with refine_iters = 0):
//   1. pn_solve_kernel          one thread per iteration: counter-based sample of 4 distinct indices, P3P on the first three
//                               (Grunert's quartic in the depth ratio, its positive roots bracketed between the critical
//                               points and bisected, three Newton steps on the three distance equations, the rigid motion
//                               of the two triangles), the fourth point chooses among the solutions
//   2. rs_count_kernel<PnModel> grid (max_iters slots) x (2048-point chunks): reprojection error in front of the camera
//   3. rs_select_kernel<4, 1>   the sequential selection loop replayed on the counts
//   4. rs_mask_kernel<PnModel>  the chosen candidate's mask; (the model's tail) R_out, t_out, info[4..7], the refit's state
//      (2 - 4: ransac.h's frame on the model PnModel, as is the sampler of 1)
//   5. the refit chain, pairs of rf_accum_kernel<PnTerms> (per 2048-point chunk: 29 sums over the mask, every thread over
//      its points in order, every wavefront in a fixed tree, the 4 wavefronts in order -> scratch) and pn_finish_kernel (one
//      workgroup: the chunks in chunk order, then rf_step: accept or undo the last step, take the next); refit.h's frame.
//      A device-side flag ends the chain's work early; its length never depends on the data.
// A candidate is 9 doubles: rows 1 and 2 of R, then t; row 3 is their cross product wherever the candidate is used.
// No floating-point atomics: the same input gives the same bits.  No host waits, no allocation: capturable.
// Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "handleless.h"
#include "pinhole.h"
#include "ransac.h"
#include "refit.h"

using namespace cotr_detail;

#define PN_MODEL 4
#define PN_SUMS 29             // 21 of J^T J, 6 of J^T r, the squared error, the inliers behind the camera
#define PN_MAX_REFINE 64
#define PN_POLISH 3            // Newton steps on every solution
#define PN_BISECT 128          // bisection steps allowed per root (an interval of doubles is exhausted well before)
#define PN_VMAX 1e8            // the depth ratios looked at: (0, PN_VMAX)
#define PN_SAMPLE_TOL 1e-18    // (1e-9 px)^2: a solution must put its three sample points back this close

// ---- a candidate ------------------------------------------------------------------------------------------------------
// m[9] = rows 1 and 2 of R, t -> the camera-space point of X (row 3 of R: the cross product of the two)
RS_HD __forceinline__ void pn_transform(const double* m, double X, double Y, double Z, double* x, double* y, double* z) {
  const double r20 = m[1] * m[5] - m[2] * m[4], r21 = m[2] * m[3] - m[0] * m[5], r22 = m[0] * m[4] - m[1] * m[3];
  *x = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[6];
  *y = ((m[3] * X + m[4] * Y) + m[5] * Z) + m[7];
  *z = ((r20 * X + r21 * Y) + r22 * Z) + m[8];
}

// the pixel of the camera-space point (x, y, z)
RS_HD __forceinline__ void pn_project(const EsCam& k, double x, double y, double z, double* u, double* v) {
  const double xn = x / z, yn = y / z;
  *u = (k.fx * xn + k.s * yn) + k.cx;
  *v = k.fy * yn + k.cy;
}

// squared reprojection error of X against the pixel (u, v); false unless X lies in front of the camera
RS_HD __forceinline__ bool pn_error(const double* m, const EsCam& k, double X, double Y, double Z, double u, double v, double* err) {
  double x, y, z, pu, pv;
  pn_transform(m, X, Y, Z, &x, &y, &z);
  if (!(z > 0.0)) return false;   // also for NaN
  pn_project(k, x, y, z, &pu, &pv);
  const double dx = pu - u, dy = pv - v;
  *err = dx * dx + dy * dy;
  return true;
}

// the refit's state, in scratch, and the model of refit.h's step: exp([w]x) R, t + dt
struct PnState : RfPose {
  static constexpr int PARAMS = 6;
  // no inlier behind the camera
  static __device__ __forceinline__ bool acceptable(const PnState*, const double* sums) { return sums[28] == 0.0; }
  static __device__ __forceinline__ void apply(PnState* st, const double* d) {
    rotate(st, d);
    for (int i = 0; i < 3; ++i) st->t[i] = st->t[i] + d[3 + i];
  }
};

// the model of ransac.h's frame: one candidate per 4-point sample; the tail writes the chosen pose and starts the refit
struct PnModel {
  static constexpr int MODEL = PN_MODEL, SLOTS = 1;
  struct Points {
    const double* __restrict__ obj;
    const double* __restrict__ img;
    EsCam k;
  };
  struct Tail {
    const double* cand;
    int32_t* info;
    double* R_out;
    double* t_out;
    PnState* st;
  };

  static __device__ __forceinline__ bool inlier(const double* m, const Points& pts, int p, float thr) {
    const double* X = pts.obj + (size_t)p * 3;
    const double u = f32r(pts.img[(size_t)p * 2]), v = f32r(pts.img[(size_t)p * 2 + 1]);
    double err;
    if (!pn_error(m, pts.k, X[0], X[1], X[2], u, v, &err)) return false;
    return (float)err <= thr;   // false for NaN
  }

  static __device__ __forceinline__ void tail(const Tail& t, int found) {
    double m[9];
    for (int i = 0; i < 9; ++i) m[i] = found ? t.cand[(size_t)t.info[3] * 9 + i] : 0.0;
    double R[9];
    for (int i = 0; i < 6; ++i) R[i] = m[i];
    R[6] = m[1] * m[5] - m[2] * m[4], R[7] = m[2] * m[3] - m[0] * m[5], R[8] = m[0] * m[4] - m[1] * m[3];
    for (int i = 0; i < 9; ++i) t.R_out[i] = t.st->R[i] = R[i];
    for (int i = 0; i < 3; ++i) t.t_out[i] = t.st->t[i] = m[6 + i];
    t.st->done = found ? 0 : 1;
    t.st->kept = 0;
    t.st->trial = 0;
    for (int i = 4; i < 8; ++i) t.info[i] = 0;
  }
};

// ---- P3P ------------------------------------------------------------------------------------------------------------------
template <int DEG>
RS_HD __forceinline__ double pn_poly(const double* c, double x) {   // c[0] x^DEG + ... + c[DEG]
  double r = c[0];
#pragma unroll
  for (int i = 1; i <= DEG; ++i) r = r * x + c[i];
  return r;
}

// The polynomial is monotone on [lo, hi]: its root there by bisection when the signs at the ends differ (a zero at lo
// counts, a zero at hi belongs to the next interval); otherwise lo, and hit = false.
template <int DEG>
RS_HD __forceinline__ double pn_bisect(const double* c, double lo, double hi, bool* hit) {
  const double flo = pn_poly<DEG>(c, lo), fhi = pn_poly<DEG>(c, hi);
  *hit = (flo <= 0.0 && fhi > 0.0) || (flo >= 0.0 && fhi < 0.0);   // false for NaN
  if (!*hit || flo == 0.0) return lo;
  const bool neg = flo < 0.0;
  for (int i = 0; i < PN_BISECT; ++i) {
    const double mid = 0.5 * (lo + hi);
    if (!(mid > lo && mid < hi)) break;
    const double fm = pn_poly<DEG>(c, mid);
    if ((fm < 0.0) == neg && fm != 0.0) lo = mid;
    else hi = mid;
  }
  return 0.5 * (lo + hi);
}

// x when it is a number, kept inside [lo, hi]; lo otherwise
RS_HD __forceinline__ double pn_clamp(double x, double lo, double hi) { return x == x ? fmin(fmax(x, lo), hi) : lo; }

// P3P on the object points X0, X1, X2 (Xo[k * 3 + i]) and their pixels (rounded to float32 by the caller), the fourth pair
// choosing: every root v = s2 / s0 in (0, PN_VMAX) of Grunert's quartic in ascending order, with u = s1 / s0 from the
// difference of two of the distance equations and s0 from the third; PN_POLISH Newton steps on the three equations
//   s1^2 + s2^2 - 2 s1 s2 cos(f1, f2) = |X1 - X2|^2,  s0^2 + s2^2 - 2 s0 s2 cos(f0, f2) = |X0 - X2|^2,
//   s0^2 + s1^2 - 2 s0 s1 cos(f0, f1) = |X0 - X1|^2
// (f: the unit bearings K^-1 (u, v, 1)); a solution needs three positive depths; its pose is the rigid motion that takes the
// orthonormal frame of the object triangle to that of the triangle s_k f_k, and it must put the three sample points back
// within 1e-9 px.  Of the solutions with the fourth point in front of the camera, the one with the smallest squared
// reprojection error there (the first of equal ones) -> best[9]; false when there is none.
RS_HD __forceinline__ bool pn_p3p(const double* Xo, const double* px, const double* py, const EsCam& k, double* best) {
  // the object triangle: edges, collinearity, frame
  const double e1x = Xo[3] - Xo[0], e1y = Xo[4] - Xo[1], e1z = Xo[5] - Xo[2];
  const double e2x = Xo[6] - Xo[0], e2y = Xo[7] - Xo[1], e2z = Xo[8] - Xo[2];
  const double e3x = Xo[6] - Xo[3], e3y = Xo[7] - Xo[4], e3z = Xo[8] - Xo[5];
  const double c2 = e1x * e1x + e1y * e1y + e1z * e1z, b2 = e2x * e2x + e2y * e2y + e2z * e2z, a2 = e3x * e3x + e3y * e3y + e3z * e3z;
  const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  const double nn = sqrt(nx * nx + ny * ny + nz * nz), l1 = sqrt(c2), l2 = sqrt(b2);
  if (!(nn > RS_RANK_TOL * (l1 * l2))) return false;   // collinear (or NaN)
  const double o1x = e1x / l1, o1y = e1y / l1, o1z = e1z / l1;
  const double o3x = nx / nn, o3y = ny / nn, o3z = nz / nn;
  const double o2x = o3y * o1z - o3z * o1y, o2y = o3z * o1x - o3x * o1z, o2z = o3x * o1y - o3y * o1x;
  // unit bearings
  double fx[3], fy[3], fz[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double yn = (py[i] - k.cy) / k.fy;
    const double xn = (px[i] - k.cx - k.s * yn) / k.fx;
    const double nrm = sqrt(xn * xn + yn * yn + 1.0);
    fx[i] = xn / nrm, fy[i] = yn / nrm, fz[i] = 1.0 / nrm;
  }
  const double ca = fx[1] * fx[2] + fy[1] * fy[2] + fz[1] * fz[2];
  const double cb = fx[0] * fx[2] + fy[0] * fy[2] + fz[0] * fz[2];
  const double cg = fx[0] * fx[1] + fy[0] * fy[1] + fz[0] * fz[1];
  // 2 u (cg - v ca) = N(v) = (K - 1) v^2 - 2 K cb v + (1 + K), K = (a2 - c2) / b2; with D = 2 (cg - v ca) and
  // G = 1 - (c2 / b2)(1 + v^2 - 2 v cb): the quartic N^2 - 2 cg N D + G D^2
  const double K = (a2 - c2) / b2, q = c2 / b2;
  const double n2 = K - 1.0, n1 = -2.0 * K * cb, n0 = 1.0 + K;
  const double d1 = -2.0 * ca, d0 = 2.0 * cg;
  const double g2 = -q, g1 = 2.0 * q * cb, g0 = 1.0 - q;
  const double dd2 = d1 * d1, dd1 = 2.0 * d1 * d0, dd0 = d0 * d0;
  const double m2 = -2.0 * cg;
  double p[5];
  p[0] = n2 * n2 + g2 * dd2;
  p[1] = 2.0 * n2 * n1 + m2 * (n2 * d1) + (g2 * dd1 + g1 * dd2);
  p[2] = (n1 * n1 + 2.0 * n2 * n0) + m2 * (n2 * d0 + n1 * d1) + ((g2 * dd0 + g1 * dd1) + g0 * dd2);
  p[3] = 2.0 * n1 * n0 + m2 * (n1 * d0 + n0 * d1) + (g1 * dd0 + g0 * dd1);
  p[4] = n0 * n0 + m2 * (n0 * d0) + g0 * dd0;
  // every root lies below the Cauchy bound; the monotone pieces of the quartic on [0, B] lie between the roots of its
  // derivative there, whose monotone pieces lie between the roots of the second derivative
  double B = 1.0 + fmax(fmax(fabs(p[1]), fabs(p[2])), fmax(fabs(p[3]), fabs(p[4]))) / fabs(p[0]);
  if (!(B < PN_VMAX)) B = PN_VMAX;
  const double dq[3] = {12.0 * p[0], 6.0 * p[1], 2.0 * p[2]};
  const double dc[4] = {4.0 * p[0], 3.0 * p[1], 2.0 * p[2], p[3]};
  double qa = NAN, qb = NAN;
  {
    const double disc = dq[1] * dq[1] - 4.0 * dq[0] * dq[2];
    if (disc >= 0.0) {
      const double h = -0.5 * (dq[1] + copysign(sqrt(disc), dq[1]));
      const double r1 = h / dq[0], r2 = dq[2] / h;   // NaN or infinite where a division is by 0: dropped by pn_clamp or kept at B
      qa = fmin(r1, r2), qb = fmax(r1, r2);
      if (!(r1 == r1) || !(r2 == r2)) qa = qb = NAN;
    }
  }
  double e[4];
  e[0] = 0.0, e[1] = pn_clamp(qa, 0.0, B), e[2] = pn_clamp(qb, e[1], B), e[3] = B;
  double g[5];
  g[0] = 0.0, g[4] = B;
  bool hit;
#pragma unroll
  for (int i = 0; i < 3; ++i) g[i + 1] = pn_bisect<3>(dc, e[i], e[i + 1], &hit);
  bool any = false;
  double best_err = INFINITY;
#pragma unroll 1
  for (int i = 0; i < 4; ++i) {
    double lo = g[0], hi = g[1];
    lo = i == 1 ? g[1] : lo, hi = i == 1 ? g[2] : hi;
    lo = i == 2 ? g[2] : lo, hi = i == 2 ? g[3] : hi;
    lo = i == 3 ? g[3] : lo, hi = i == 3 ? g[4] : hi;
    const double v = pn_bisect<4>(p, lo, hi, &hit);
    if (!hit || !(v > 0.0)) continue;
    const double u = ((n2 * v + n1) * v + n0) / (d1 * v + d0);
    double s0 = sqrt(b2 / ((1.0 + v * v) - 2.0 * v * cb));
    double s1 = u * s0, s2 = v * s0;
#pragma unroll 1
    for (int st = 0; st < PN_POLISH; ++st) {
      const double F0 = ((s1 * s1 + s2 * s2) - 2.0 * (s1 * s2) * ca) - a2;
      const double F1 = ((s0 * s0 + s2 * s2) - 2.0 * (s0 * s2) * cb) - b2;
      const double F2 = ((s0 * s0 + s1 * s1) - 2.0 * (s0 * s1) * cg) - c2;
      // J = [0 A B; C 0 D; E F 0]
      const double A = 2.0 * (s1 - s2 * ca), Bq = 2.0 * (s2 - s1 * ca);
      const double C = 2.0 * (s0 - s2 * cb), D = 2.0 * (s2 - s0 * cb);
      const double E = 2.0 * (s0 - s1 * cg), F = 2.0 * (s1 - s0 * cg);
      const double det = A * (D * E) + Bq * (C * F);
      if (!(fabs(det) > 0.0) || !(fabs(det) < INFINITY)) break;
      // the adjugate of J applied to F
      const double x0 = ((-(D * F)) * F0 + (Bq * F) * F1 + (A * D) * F2) / det;
      const double x1 = ((D * E) * F0 + (-(Bq * E)) * F1 + (Bq * C) * F2) / det;
      const double x2 = ((C * F) * F0 + (A * E) * F1 + (-(A * C)) * F2) / det;
      s0 = s0 - x0, s1 = s1 - x1, s2 = s2 - x2;
    }
    if (!(s0 > 0.0 && s1 > 0.0 && s2 > 0.0)) continue;   // also for NaN
    // the camera triangle and its frame
    const double y0x = s0 * fx[0], y0y = s0 * fy[0], y0z = s0 * fz[0];
    const double h1x = s1 * fx[1] - y0x, h1y = s1 * fy[1] - y0y, h1z = s1 * fz[1] - y0z;
    const double h2x = s2 * fx[2] - y0x, h2y = s2 * fy[2] - y0y, h2z = s2 * fz[2] - y0z;
    const double hl = sqrt(h1x * h1x + h1y * h1y + h1z * h1z);
    const double mx = h1y * h2z - h1z * h2y, my = h1z * h2x - h1x * h2z, mz = h1x * h2y - h1y * h2x;
    const double mn = sqrt(mx * mx + my * my + mz * mz);
    const double c1x = h1x / hl, c1y = h1y / hl, c1z = h1z / hl;
    const double c3x = mx / mn, c3y = my / mn, c3z = mz / mn;
    const double c2x = c3y * c1z - c3z * c1y, c2y = c3z * c1x - c3x * c1z;
    // rows 1 and 2 of R = c1 o1^T + c2 o2^T + c3 o3^T, t = Y0 - R X0 with row 3 as every user rebuilds it
    double m[9];
    m[0] = (c1x * o1x + c2x * o2x) + c3x * o3x, m[1] = (c1x * o1y + c2x * o2y) + c3x * o3y, m[2] = (c1x * o1z + c2x * o2z) + c3x * o3z;
    m[3] = (c1y * o1x + c2y * o2x) + c3y * o3x, m[4] = (c1y * o1y + c2y * o2y) + c3y * o3y, m[5] = (c1y * o1z + c2y * o2z) + c3y * o3z;
    (void)c1z;
    m[6] = 0.0, m[7] = 0.0, m[8] = 0.0;
    double rx, ry, rz;
    pn_transform(m, Xo[0], Xo[1], Xo[2], &rx, &ry, &rz);
    m[6] = y0x - rx, m[7] = y0y - ry, m[8] = y0z - rz;
    bool close = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double err;
      close = close && pn_error(m, k, Xo[j * 3], Xo[j * 3 + 1], Xo[j * 3 + 2], px[j], py[j], &err) && err <= PN_SAMPLE_TOL;
    }
    if (!close) continue;
    double err4;
    if (!pn_error(m, k, Xo[9], Xo[10], Xo[11], px[3], py[3], &err4)) continue;
    if (err4 < best_err) {   // false for NaN
      best_err = err4;
      any = true;
#pragma unroll
      for (int j = 0; j < 9; ++j) best[j] = m[j];
    }
  }
  return any;
}

__global__ __launch_bounds__(RS_SOLVE_THREADS) void pn_solve_kernel(const double* __restrict__ obj, const double* __restrict__ img, int n,
                                                                    EsCam k, int max_iters, uint64_t seed, double* __restrict__ Pc,
                                                                    int* __restrict__ count, double* __restrict__ hyp_pose,
                                                                    int32_t* __restrict__ hyp_samples) {
  __shared__ int shI[PN_MODEL * RS_SOLVE_THREADS];   // the sample: the sampler indexes it at run time
  const int lane = threadIdx.x;
  const int it = blockIdx.x * RS_SOLVE_THREADS + lane;
  if (it >= max_iters) return;   // no workgroup barrier below
#define S_(k) shI[(k) * RS_SOLVE_THREADS + lane]
  const int got = rs_sample<PN_MODEL>(seed, it, n, &shI[lane], RS_SOLVE_THREADS);
  if (hyp_samples) {
    for (int j = 0; j < PN_MODEL; ++j) hyp_samples[(size_t)it * PN_MODEL + j] = j < got ? S_(j) : -1;
  }
  bool ok = got == PN_MODEL;
  double m[9];
  if (ok) {
    double Xo[12], px[4], py[4];
    bool finite = true;
#pragma unroll
    for (int j = 0; j < PN_MODEL; ++j) {
      const int i = S_(j);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        Xo[j * 3 + c] = obj[(size_t)i * 3 + c];
        finite = finite && Xo[j * 3 + c] == Xo[j * 3 + c];
      }
      px[j] = f32r(img[(size_t)i * 2]), py[j] = f32r(img[(size_t)i * 2 + 1]);
      finite = finite && px[j] == px[j] && py[j] == py[j];
    }
    ok = finite && pn_p3p(Xo, px, py, k, m);
  }
#undef S_
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const double v = ok ? m[i] : NAN;   // a slot without a candidate: NaN, count -1
    Pc[(size_t)it * 9 + i] = v;
    if (hyp_pose) hyp_pose[(size_t)it * 9 + i] = v;
  }
  count[it] = ok ? 0 : -1;
}

// ---- the refit ------------------------------------------------------------------------------------------------------------
// One inlier's terms at the pose of st, added to acc: J^T J (21), J^T r (6), the squared error, and 1 for a point that is
// not in front of the camera (which adds nothing else).  The step is exp([w]x) R, t + dt: with P = R X the Jacobian of the
// camera-space point is [-[P]x | I].
__device__ __forceinline__ void pn_terms(const PnState* __restrict__ st, const EsCam& k, const double* X, double u, double v, double* acc) {
  const double* R = st->R;
  const double Px = (R[0] * X[0] + R[1] * X[1]) + R[2] * X[2], Py = (R[3] * X[0] + R[4] * X[1]) + R[5] * X[2],
               Pz = (R[6] * X[0] + R[7] * X[1]) + R[8] * X[2];
  const double x = Px + st->t[0], y = Py + st->t[1], z = Pz + st->t[2];
  if (!(z > 0.0)) {
    acc[28] += 1.0;
    return;
  }
  double pu, pv;
  pn_project(k, x, y, z, &pu, &pv);
  const double ru = pu - u, rv = pv - v;
  const double iz = 1.0 / z;
  // d(pu, pv) / d(x, y, z)
  const double ax = k.fx * iz, ay = k.s * iz, az = -((k.fx * x + k.s * y) * iz) * iz;
  const double by = k.fy * iz, bz = -((k.fy * y) * iz) * iz;
  // columns of -[P]x: (0, -Pz, Py), (Pz, 0, -Px), (-Py, Px, 0)
  const double j1[6] = {az * Py - ay * Pz, ax * Pz - az * Px, ay * Px - ax * Py, ax, ay, az};
  const double j2[6] = {bz * Py - by * Pz, -(bz * Px), by * Px, 0.0, by, bz};
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = i; j < 6; ++j) acc[rf_tri<6>(i, j)] += j1[i] * j1[j] + j2[i] * j2[j];
    acc[21 + i] += j1[i] * ru + j2[i] * rv;
  }
  acc[27] += ru * ru + rv * rv;
}

// the object point as it is, the pixel rounded to float32
struct PnTerms {
  static constexpr int SUMS = PN_SUMS, STRIDE = PN_SUMS;
  using Points = PnModel::Points;
  using State = PnState;
  static __device__ __forceinline__ void terms(const PnState* __restrict__ st, const Points& pts, int p, double* acc) {
    const double X[3] = {pts.obj[(size_t)p * 3], pts.obj[(size_t)p * 3 + 1], pts.obj[(size_t)p * 3 + 2]};
    pn_terms(st, pts.k, X, f32r(pts.img[(size_t)p * 2]), f32r(pts.img[(size_t)p * 2 + 1]), acc);
  }
};

// the sums of the accumulate before it: judges the step on trial, takes the next one;
// last: the chain's last launch (no further step is taken; writes R_out, t_out and info[4])
__global__ __launch_bounds__(64) void pn_finish_kernel(int chunks, const double* __restrict__ parts, PnState* __restrict__ st, int last,
                                                       double* __restrict__ R_out, double* __restrict__ t_out, int32_t* __restrict__ info) {
  __shared__ double sums[PN_SUMS];
  const bool active = !st->done;   // uniform; read before anything below writes it
  rf_reduce<PN_SUMS>(parts, chunks, active ? PN_SUMS : 0, sums);
  if (threadIdx.x != 0) return;
  if (active) rf_step(st, sums, last);
  if (last) {
    const int found = info[0];
    for (int i = 0; i < 9; ++i) R_out[i] = found ? st->R[i] : 0.0;
    for (int i = 0; i < 3; ++i) t_out[i] = found ? st->t[i] : 0.0;
    info[4] = st->kept;
  }
}

// ---- the lift -------------------------------------------------------------------------------------------------------------
// One thread per point: the depth at the pixel the point falls in (es_nearest), X = z K^-1 (x, y, 1) with the point as
// it is (es_ray), then c2w (es_to_world) when given; three NaN outside the map or without a finite depth > 0.
__global__ __launch_bounds__(256) void pn_lift_kernel(const float* __restrict__ depth, int H, int W, EsCam k, const double* __restrict__ c2w,
                                                      const double* __restrict__ pts, int n, double* __restrict__ out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const double x = pts[(size_t)p * 2], y = pts[(size_t)p * 2 + 1];
  int px, py;
  double X[3] = {NAN, NAN, NAN};
  if (es_nearest(x, y, H, W, &px, &py)) {
    const double z = (double)depth[(size_t)py * W + px];
    if (z > 0.0 && z < INFINITY) {
      double xn, yn;
      es_ray(k, x, y, &xn, &yn);
      const double c[3] = {xn * z, yn * z, z};
      if (c2w)
        es_to_world(c2w, c, X);
      else
        X[0] = c[0], X[1] = c[1], X[2] = c[2];
    }
  }
  out[(size_t)p * 3] = X[0], out[(size_t)p * 3 + 1] = X[1], out[(size_t)p * 3 + 2] = X[2];
}

// ---- host side ------------------------------------------------------------------------------------------------------------
namespace {

const RsEntry PN_ENTRY = {"cotr_ransac_pnp", "R_out", PN_MODEL, "", PnModel::SLOTS, RS_MAX_ITERS};

// after the frame's candidates and counts: the refit's state, then its partial sums [chunks, PN_SUMS]
RfPlan pn_plan(const RsPlan& rs, int n) { return rf_plan(rs.bytes, sizeof(PnState), n, PN_SUMS); }

}  // namespace

extern "C" {

int cotr_lift_pixels(const float* depth, int H, int W, const double* K, const double* c2w, const double* points, int n, double* out,
                     cotr_stream stream) {
  if (H < 1 || W < 1 || (long long)H * W > MAX_PIXELS) return handleless_fail(COTR_ERR_ARG, "cotr_lift_pixels: H and W must be >= 1 with at most 2^28 pixels");
  if (n < 1 || n > RS_MAX_POINTS) return handleless_fail(COTR_ERR_ARG, "cotr_lift_pixels: n must be in [1, 2^24]");
  if (!depth || !K || !points || !out) return handleless_fail(COTR_ERR_ARG, "cotr_lift_pixels: depth, K, points and out must not be NULL");
  EsCam k;
  if (!es_camera(K, &k)) return handleless_fail(COTR_ERR_ARG, "cotr_lift_pixels: the camera matrix must be finite with focal lengths that are not 0");
  if (!aligned(depth, 4) || !aligned(c2w, 8) || !aligned(points, 8) || !aligned(out, 8))
    return handleless_fail(COTR_ERR_ARG, "cotr_lift_pixels: floats must be 4-byte and doubles 8-byte aligned");
  hipLaunchKernelGGL(pn_lift_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), depth, H, W, k, c2w,
                     points, n, out);
  return launched();
}

int cotr_ransac_pnp_scratch_bytes(int n, int max_iters, size_t* bytes) {
  if (const int rc = rs_scratch_bytes(PN_ENTRY, n, max_iters, bytes)) return rc;
  *bytes = pn_plan(rs_plan(PN_ENTRY, max_iters), n).bytes;
  return COTR_OK;
}

int cotr_ransac_pnp(const double* object_points, const double* image_points, int n, const double* K, double threshold, double confidence,
                    int max_iters, uint64_t seed, int refine_iters, double* R_out, double* t_out, uint8_t* mask_out, int32_t* info_out,
                    double* hyp_pose, int32_t* hyp_count, int32_t* hyp_samples, void* scratch, size_t scratch_bytes, cotr_stream stream) {
  const RsPlan rs = rs_plan(PN_ENTRY, max_iters);
  const RfPlan l = pn_plan(rs, n);
  if (const int rc = rs_check_call(PN_ENTRY, n, max_iters, threshold, confidence, object_points, image_points, R_out, mask_out, info_out,
                                   hyp_pose, hyp_count, hyp_samples, scratch, scratch_bytes, l.bytes))
    return rc;
  if (!K || !t_out) return rs_fail(PN_ENTRY, "K and t_out must not be NULL");
  if (!aligned(t_out, 8)) return rs_fail(PN_ENTRY, "t_out must be 8-byte aligned");
  if (refine_iters < 0 || refine_iters > PN_MAX_REFINE) return rs_fail(PN_ENTRY, "refine_iters must be in [0, 64]");
  EsCam k;
  if (!es_camera(K, &k)) return rs_fail(PN_ENTRY, "the camera matrix must be finite with focal lengths that are not 0");
  const float thr = (float)(threshold * threshold);
  if (!(thr > 0.0f) || !(thr < INFINITY)) return rs_fail(PN_ENTRY, "the squared threshold must be a finite float32 that is not 0");
  char* base = static_cast<char*>(scratch);
  const double* Pc = reinterpret_cast<const double*>(base + rs.candidates);
  PnState* st = reinterpret_cast<PnState*>(base + l.state);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const auto solve = [&](double* cand, int* count) {
    hipLaunchKernelGGL(pn_solve_kernel, dim3((unsigned)((max_iters + RS_SOLVE_THREADS - 1) / RS_SOLVE_THREADS)), dim3(RS_SOLVE_THREADS), 0, s,
                       object_points, image_points, n, k, max_iters, seed, cand, count, hyp_pose, hyp_samples);
  };
  const PnModel::Points pts = {object_points, image_points, k};
  rs_enqueue<PnModel>(s, solve, pts, n, max_iters, confidence, thr, rs, scratch, nullptr, mask_out, info_out, hyp_count,
                      {Pc, info_out, R_out, t_out, st});
  // pair j judges step j - 1 and takes step j; the last one takes none
  for (int j = 0; refine_iters > 0 && j <= refine_iters; ++j)
    rf_enqueue_pair<PnTerms>(s, l, scratch, pts, n, mask_out, pn_finish_kernel, (int)(j == refine_iters), R_out, t_out, info_out);
  return launched();
}

}  // extern "C"
