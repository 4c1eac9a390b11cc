// Essential-matrix RANSAC (five-point minimal solver) and the pose of an essential matrix, in the structure of OpenCV's
// findEssentialMat(RANSAC) + recoverPose.  Rules in DESIGN.md 3h-3.  x2h^T E x1h = 0 on camera-normalised points.
//
// cotr_ransac_essential: 5 launches on the caller's stream:
//   1. es_normalise_kernel  the points rounded to float32, then through the inverse camera matrices (float64) -> scratch
//   2. es_solve_kernel          one thread per iteration, 32 per workgroup: counter-based sample of 5 distinct indices, the
//                               five-point solver in per-thread LDS columns -> 0..10 candidates in slots 10 * it + k
//   3. rs_count_kernel<EsModel> grid (10 * max_iters slots) x (2048-point chunks): Sampson error
//   4. rs_select_kernel<5, 10>  the sequential selection loop replayed on the counts
//   5. rs_mask_kernel<EsModel>  the chosen candidate and its mask; (the model's tail) info[4..7] = 0
//      (3 - 5: ransac.h's frame on the model EsModel, as are the sampler and the elimination of the 5 x 9 system)
// cotr_recover_pose: 3 launches:
//   1. es_decompose_kernel  one workgroup: V from cyclic Jacobi on E^T E (ransac.h), U, the two rotations and t
//   2. es_front_kernel      per 2048-point chunk: the least-squares depths of every masked point under the four candidates,
//                           ballot + popcount, four integer atomics per wavefront
//   3. es_pose_kernel       the first candidate with the largest count: R, t, info and mask_out
// cotr_refine_pose (rules in DESIGN.md 3h-5): 2 + rounds * (1 + 2 * (refine_iters + 1)) launches:
//   1. es_normalise_kernel  as above
//   2. rp_init_kernel       one thread: the state (R, unit t, E = [t]x R and its five directional derivatives)
//   per round:
//   3. rp_mask_kernel       per 2048-point chunk: the round's mask (round 1: mask_in; later: Sampson inliers of E in front
//                           under (R, t)) and its integer count
//   4. refine_iters + 1 pairs of rf_accum_kernel<RpTerms> (per chunk: 22 sums over the mask, every thread over its points in
//      order, every wavefront in a fixed tree, the 4 wavefronts in order -> scratch) and rp_finish_kernel (one workgroup: the
//      chunks in chunk order, then rf_step: accept or undo the last step, take the next; the round's last takes none, the
//      call's last writes the outputs); refit.h's frame.  A device-side flag idles the rest of a round's chain; its length
//      never depends on the data.
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

#define ES_MODEL 5
#define ES_SLOTS 10
#define ES_SOLVE_THREADS 32    // samples per workgroup: 32 x (222 doubles + 15 ints) = 58752 bytes of static LDS
#define ES_MAX_ITERS 6553      // 10 * max_iters slots stay under rs_select_kernel's 65536
#define ES_POLISH 3            // Gauss-Newton steps on every root
#define ES_QR_SWEEPS 30        // QR sweeps allowed per eigenvalue
#define ES_DOUBLES 222         // per-sample LDS: the 10 x 20 system, 10 real roots, 12 of small systems
#define ES_INTS 15             // the sample, a column permutation

// ---- polynomials in (x, y, z, w = 1) --------------------------------------------------------------------------------
// a linear one has 4 coefficients (x, y, z, 1), a quadratic one 10 (pairs i <= j at es_q2), a cubic one 20, in the column
// order of the 10 x 20 system: x3 x2y xy2 y3 x2z xyz y2z xz2 yz2 z3 | x2 xy y2 xz yz z2 x y z 1
ES_HD constexpr int es_q2(int i, int j) { return i <= j ? i * 4 - i * (i - 1) / 2 + (j - i) : j * 4 - j * (j - 1) / 2 + (i - j); }

ES_HD constexpr int es_col(int i, int j, int k) {
  const int ex = (i == 0) + (j == 0) + (k == 0), ey = (i == 1) + (j == 1) + (k == 1), ez = (i == 2) + (j == 2) + (k == 2);
  const int key = ex * 16 + ey * 4 + ez;
  const int keys[20] = {48, 36, 24, 12, 33, 21, 9, 18, 6, 3, 32, 20, 8, 17, 5, 2, 16, 4, 1, 0};
  for (int c = 0; c < 20; ++c)
    if (keys[c] == key) return c;
  return -1;
}

// q += sign * a * b
ES_HD __forceinline__ void es_mul11(const double* a, const double* b, double sign, double* q) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) q[es_q2(i, j)] += sign * (a[i] * b[j]);
}

// c += q * l
ES_HD __forceinline__ void es_mul21(const double* q, const double* l, double* c) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = i; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < 4; ++k) c[es_col(i, j, k)] += q[es_q2(i, j)] * l[k];
}

// ---- the 3 x 3 solve of the polish step ---------------------------------------------------------------------------------
// rs_solve<3, STRIDE> of ransac.h written out (the same rule, operation for operation; a: the augmented 3 x 4 system).  Kept
// in this form for es_solve_kernel alone, which sits at the register limit: with the shared template, the same arithmetic
// inlined in another shape, it spills two registers more (164 -> 172 bytes of scratch per lane) in its hottest loop.
template <int STRIDE>
ES_HD bool es_solve3(double* a, int* perm, double* z) {
  constexpr int N = 3;
#define A_(r, c) a[((r) * (N + 1) + (c)) * STRIDE]
#define P_(c) perm[(c) * STRIDE]
  for (int c = 0; c < N; ++c) P_(c) = c;
  double piv0 = 0.0;
  for (int k = 0; k < N; ++k) {
    double pv = -1.0;
    int pr = k, pc = k;
    for (int r = k; r < N; ++r)
      for (int c = k; c < N; ++c) {
        const double v = fabs(A_(r, c));
        if (v > pv) pv = v, pr = r, pc = c;
      }
    if (k == 0) piv0 = pv;
    if (!(pv > RS_RANK_TOL * piv0)) return false;   // also for NaN
    if (pr != k)
      for (int c = 0; c < N + 1; ++c) {
        const double t = A_(k, c);
        A_(k, c) = A_(pr, c);
        A_(pr, c) = t;
      }
    if (pc != k) {
      for (int r = 0; r < N; ++r) {
        const double t = A_(r, k);
        A_(r, k) = A_(r, pc);
        A_(r, pc) = t;
      }
      const int t = P_(k);
      P_(k) = P_(pc);
      P_(pc) = t;
    }
    const double akk = A_(k, k);
    for (int r = k + 1; r < N; ++r) {
      const double m = A_(r, k) / akk;
      for (int c = k + 1; c < N + 1; ++c) A_(r, c) = A_(r, c) - m * A_(k, c);
      A_(r, k) = 0.0;
    }
  }
  double y[N];
#pragma unroll
  for (int r = N - 1; r >= 0; --r) {
    double acc = A_(r, N);
#pragma unroll
    for (int c = r + 1; c < N; ++c) acc -= A_(r, c) * y[c];
    y[r] = acc / A_(r, r);
  }
  // z[perm[c]] = y[c], without indexing registers at run time
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double v = 0.0;
#pragma unroll
    for (int c = 0; c < N; ++c) v = P_(c) == i ? y[c] : v;
    z[i] = v;
  }
#undef A_
#undef P_
  return true;
}

// ---- the five-point solver ------------------------------------------------------------------------------------------
// Per-sample memory: mem[e * STRIDE], e < ES_DOUBLES; perm[c * STRIDE], c < 10.
#define M_(r, c) mem[((r) * 20 + (c)) * STRIDE]          // the 10 x 20 system; its left half later holds 10 x 10 matrices
#define Q_(r, c) mem[((r) * 9 + (c)) * STRIDE]           // the 5 x 9 epipolar system (before the 10 x 20 one)
#define NS_(t, i) mem[(100 + (t) * 9 + (i)) * STRIDE]    // the null-space basis on its way to registers
#define WR_(k) mem[(200 + (k)) * STRIDE]                 // real roots
#define T_(k) mem[(210 + (k)) * STRIDE]                  // a null vector, or the 3 x 4 system of a polish step
#define P_(c) perm[(c) * STRIDE]

// The left half of M_ <- the action matrix of multiplication by x on the basis x2 xy y2 xz yz z2 x y z 1, minus shift on
// the diagonal.  The right half of M_ holds B of the reduced system [I | B].
template <int STRIDE>
ES_HD __forceinline__ void es_action(double* mem, double shift) {
  const int rows[6] = {0, 1, 2, 4, 5, 7};   // x * (x2 xy y2 xz yz z2) = x3 x2y xy2 x2z xyz xz2
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 10; ++j) M_(i, j) = -M_(rows[i], 10 + j);
  for (int i = 6; i < 10; ++i)
    for (int j = 0; j < 10; ++j) M_(i, j) = 0.0;
  M_(6, 0) = 1.0, M_(7, 1) = 1.0, M_(8, 3) = 1.0, M_(9, 6) = 1.0;   // x * (x y z 1) = x2 xy xz x
  for (int i = 0; i < 10; ++i) M_(i, i) = M_(i, i) - shift;
}

// The real eigenvalues of the 10 x 10 matrix in the left half of M_ (destroyed): reduction to Hessenberg form by
// elimination with pivoting, then the double-shift QR iteration (the EISPACK elmhes / hqr scheme) -> WR_, how many; -1
// when an eigenvalue takes more than ES_QR_SWEEPS sweeps.
template <int STRIDE>
ES_HD int es_real_eigenvalues(double* mem) {
  const int n = 10;
  for (int m = 1; m < n - 1; ++m) {
    double x = 0.0;
    int i = m;
    for (int j = m; j < n; ++j)
      if (fabs(M_(j, m - 1)) > fabs(x)) x = M_(j, m - 1), i = j;
    if (i != m) {
      for (int j = m - 1; j < n; ++j) {
        const double t = M_(i, j);
        M_(i, j) = M_(m, j);
        M_(m, j) = t;
      }
      for (int j = 0; j < n; ++j) {
        const double t = M_(j, i);
        M_(j, i) = M_(j, m);
        M_(j, m) = t;
      }
    }
    if (x != 0.0)
      for (i = m + 1; i < n; ++i) {
        double y = M_(i, m - 1);
        if (y != 0.0) {
          y = y / x;
          // whole rows and columns through registers, so that their LDS reads are in flight together
          double a[10], b[10];
#pragma unroll
          for (int j = 0; j < 10; ++j) a[j] = M_(i, j), b[j] = M_(m, j);
#pragma unroll
          for (int j = 0; j < 10; ++j) M_(i, j) = j >= m ? a[j] - y * b[j] : a[j];
#pragma unroll
          for (int j = 0; j < 10; ++j) a[j] = M_(j, m), b[j] = M_(j, i);
#pragma unroll
          for (int j = 0; j < 10; ++j) M_(j, m) = a[j] + y * b[j];
        }
      }
  }
  for (int i = 2; i < n; ++i)
    for (int j = 0; j < i - 1; ++j) M_(i, j) = 0.0;
  double anorm = 0.0;
  for (int i = 0; i < n; ++i)
    for (int j = i > 0 ? i - 1 : 0; j < n; ++j) anorm += fabs(M_(i, j));
  int nreal = 0, nn = n - 1, its = 0;
  double t = 0.0;
  while (nn >= 0) {
    int l;
    for (l = nn; l >= 1; --l) {
      double s = fabs(M_(l - 1, l - 1)) + fabs(M_(l, l));
      if (s == 0.0) s = anorm;
      if (fabs(M_(l, l - 1)) + s == s) {
        M_(l, l - 1) = 0.0;
        break;
      }
    }
    double x = M_(nn, nn);
    if (l == nn) {   // one root
      WR_(nreal) = x + t;
      ++nreal;
      nn -= 1;
      its = 0;
      continue;
    }
    double y = M_(nn - 1, nn - 1), w = M_(nn, nn - 1) * M_(nn - 1, nn);
    if (l == nn - 1) {   // two roots: real when the discriminant is not negative
      const double p = 0.5 * (y - x), q = p * p + w;
      if (q >= 0.0) {
        const double z = p + copysign(sqrt(q), p);
        x += t;
        WR_(nreal) = x + z;
        WR_(nreal + 1) = z != 0.0 ? x - w / z : x + z;
        nreal += 2;
      }
      nn -= 2;
      its = 0;
      continue;
    }
    if (its == ES_QR_SWEEPS || !(anorm < INFINITY)) return -1;   // (also for a NaN matrix)
    if (its == 10 || its == 20) {   // an exceptional shift
      t += x;
      for (int i = 0; i <= nn; ++i) M_(i, i) = M_(i, i) - x;
      const double s = fabs(M_(nn, nn - 1)) + fabs(M_(nn - 1, nn - 2));
      x = y = 0.75 * s;
      w = -0.4375 * s * s;
    }
    ++its;
    double p = 0.0, q = 0.0, r = 0.0, z;
    int m;
    for (m = nn - 2; m >= l; --m) {   // two consecutive small subdiagonal elements
      z = M_(m, m);
      r = x - z;
      double s = y - z;
      p = (r * s - w) / M_(m + 1, m) + M_(m, m + 1);
      q = M_(m + 1, m + 1) - z - r - s;
      r = M_(m + 2, m + 1);
      s = fabs(p) + fabs(q) + fabs(r);
      p = p / s, q = q / s, r = r / s;
      if (m == l) break;
      const double u = fabs(M_(m, m - 1)) * (fabs(q) + fabs(r));
      const double v = fabs(p) * (fabs(M_(m - 1, m - 1)) + fabs(z) + fabs(M_(m + 1, m + 1)));
      if (u + v == v) break;
    }
    for (int i = m + 2; i <= nn; ++i) {
      M_(i, i - 2) = 0.0;
      if (i != m + 2) M_(i, i - 3) = 0.0;
    }
    for (int k = m; k <= nn - 1; ++k) {   // the double QR step on rows l..nn and columns m..nn
      if (k != m) {
        p = M_(k, k - 1);
        q = M_(k + 1, k - 1);
        r = k != nn - 1 ? M_(k + 2, k - 1) : 0.0;
        x = fabs(p) + fabs(q) + fabs(r);
        if (x != 0.0) p = p / x, q = q / x, r = r / x;
      }
      const double s = copysign(sqrt(p * p + q * q + r * r), p);
      if (s != 0.0) {
        if (k == m) {
          if (l != m) M_(k, k - 1) = -M_(k, k - 1);
        } else {
          M_(k, k - 1) = -s * x;
        }
        p += s;
        x = p / s;
        y = q / s;
        z = r / s;
        q = q / p;
        r = r / p;
        // Rows k..k+2 on columns k..nn, then columns k..k+2 on rows l..min(nn, k+3): whole rows and columns through
        // registers (their LDS reads in flight together), the entries outside those ranges written back as they were.
        const bool three = k != nn - 1;
        const int k2 = three ? k + 2 : k + 1;   // without a third row or column: one inside the matrix, read and not written
        double a0[10], a1[10], a2[10];
#pragma unroll
        for (int j = 0; j < 10; ++j) a0[j] = M_(k, j), a1[j] = M_(k + 1, j), a2[j] = M_(k2, j);
#pragma unroll
        for (int j = 0; j < 10; ++j) {
          double pp = a0[j] + q * a1[j];
          if (three) pp += r * a2[j];
          const bool on = j >= k && j <= nn;
          if (three) M_(k2, j) = on ? a2[j] - pp * z : a2[j];
          M_(k + 1, j) = on ? a1[j] - pp * y : a1[j];
          M_(k, j) = on ? a0[j] - pp * x : a0[j];
        }
        const int mmin = nn < k + 3 ? nn : k + 3;
#pragma unroll
        for (int i = 0; i < 10; ++i) a0[i] = M_(i, k), a1[i] = M_(i, k + 1), a2[i] = M_(i, k2);
#pragma unroll
        for (int i = 0; i < 10; ++i) {
          double pp = x * a0[i] + y * a1[i];
          if (three) pp += z * a2[i];
          const bool on = i >= l && i <= mmin;
          if (three) M_(i, k2) = on ? a2[i] - pp * r : a2[i];
          M_(i, k + 1) = on ? a1[i] - pp * q : a1[i];
          M_(i, k) = on ? a0[i] - pp : a0[i];
        }
      }
    }
  }
  return nreal;
}

// One Gauss-Newton step on the ten constraints m3_i(p) + sum_j B[i][j] low_j(p) = 0 at p = (x, y, z); false (p kept) when
// the 3 x 3 normal equations are singular by the full-pivot rule.
template <int STRIDE>
ES_HD bool es_polish_step(double* mem, int* perm, double* p) {
  const double x = p[0], y = p[1], z = p[2];
  const double xx = x * x, xy = x * y, yy = y * y, xz = x * z, yz = y * z, zz = z * z;
  const double m3[10] = {xx * x, xx * y, x * yy, yy * y, xx * z, xy * z, yy * z, x * zz, y * zz, zz * z};
  const double d3[3][10] = {{3.0 * xx, 2.0 * xy, yy, 0.0, 2.0 * xz, yz, 0.0, zz, 0.0, 0.0},
                            {0.0, xx, 2.0 * xy, 3.0 * yy, 0.0, xz, 2.0 * yz, 0.0, zz, 0.0},
                            {0.0, 0.0, 0.0, 0.0, xx, xy, yy, 2.0 * xz, 2.0 * yz, 3.0 * zz}};
  const double low[10] = {xx, xy, yy, xz, yz, zz, x, y, z, 1.0};
  const double dl[3][10] = {{2.0 * x, y, 0.0, z, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0},
                            {0.0, x, 2.0 * y, 0.0, z, 0.0, 0.0, 1.0, 0.0, 0.0},
                            {0.0, 0.0, 0.0, x, y, 2.0 * z, 0.0, 0.0, 1.0, 0.0}};
  double JtJ[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, Jtr[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    double r = m3[i], J[3] = {d3[0][i], d3[1][i], d3[2][i]};
#pragma unroll
    for (int j = 0; j < 10; ++j) {
      const double b = M_(i, 10 + j);
      r += b * low[j];
#pragma unroll
      for (int v = 0; v < 3; ++v) J[v] += b * dl[v][j];
    }
    JtJ[0] += J[0] * J[0], JtJ[1] += J[0] * J[1], JtJ[2] += J[0] * J[2];
    JtJ[3] += J[1] * J[1], JtJ[4] += J[1] * J[2], JtJ[5] += J[2] * J[2];
#pragma unroll
    for (int v = 0; v < 3; ++v) Jtr[v] += J[v] * r;
  }
  T_(0) = JtJ[0], T_(1) = JtJ[1], T_(2) = JtJ[2], T_(3) = Jtr[0];
  T_(4) = JtJ[1], T_(5) = JtJ[3], T_(6) = JtJ[4], T_(7) = Jtr[1];
  T_(8) = JtJ[2], T_(9) = JtJ[4], T_(10) = JtJ[5], T_(11) = Jtr[2];
  double d[3];
  if (!es_solve3<STRIDE>(&T_(0), perm, d)) return false;
  p[0] = x - d[0], p[1] = y - d[1], p[2] = z - d[2];
  return true;
}

// x1, y1, x2, y2: the 5 pairs in normalised coordinates -> the candidates E (unit Frobenius norm, the first entry of
// largest magnitude positive) at out[k * 9 + i], in ascending order of the root; how many (0: the sample has no model).
template <int STRIDE>
ES_HD int es_five_point(const double* x1, const double* y1, const double* x2, const double* y2, double* mem, int* perm, double* out) {
  // 1. rows [x'x, x'y, x', y'x, y'y, y', x, y, 1]; full-pivot elimination; the 4 free (permuted) columns set to unit vectors
#pragma unroll
  for (int k = 0; k < ES_MODEL; ++k) {
    Q_(k, 0) = x2[k] * x1[k], Q_(k, 1) = x2[k] * y1[k], Q_(k, 2) = x2[k];
    Q_(k, 3) = y2[k] * x1[k], Q_(k, 4) = y2[k] * y1[k], Q_(k, 5) = y2[k];
    Q_(k, 6) = x1[k], Q_(k, 7) = y1[k], Q_(k, 8) = 1.0;
  }
  if (!rs_eliminate<ES_MODEL, 9, 9, STRIDE>(&Q_(0, 0), perm)) return 0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    double z[9];
    rs_null_vector<ES_MODEL, 9, STRIDE>(&Q_(0, 0), ES_MODEL + t, z);
#pragma unroll
    for (int c = 0; c < 9; ++c) NS_(t, P_(c)) = z[c];
  }
  // the basis, orthonormalised (modified Gram-Schmidt): El[e][v], E = x El[.][0] + y El[.][1] + z El[.][2] + El[.][3]
  double El[9][4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
#pragma unroll
    for (int e = 0; e < 9; ++e) El[e][t] = NS_(t, e);
#pragma unroll
    for (int s = 0; s < t; ++s) {
      double d = 0.0;
#pragma unroll
      for (int e = 0; e < 9; ++e) d += El[e][s] * El[e][t];
#pragma unroll
      for (int e = 0; e < 9; ++e) El[e][t] = El[e][t] - d * El[e][s];
    }
    double ss = 0.0;
#pragma unroll
    for (int e = 0; e < 9; ++e) ss += El[e][t] * El[e][t];
    const double nrm = sqrt(ss);
#pragma unroll
    for (int e = 0; e < 9; ++e) El[e][t] = El[e][t] / nrm;
  }
  // 2. the ten cubic constraints, each row scaled to unit norm: (E E^T - tr(E E^T) / 2 I) E (9 rows) and det E
  {
    double L[6][10];   // the symmetric E E^T - tr / 2 I: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
    const int lr[6] = {0, 0, 0, 1, 1, 2}, lc[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
    for (int s = 0; s < 6; ++s) {
#pragma unroll
      for (int m = 0; m < 10; ++m) L[s][m] = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) es_mul11(El[lr[s] * 3 + k], El[lc[s] * 3 + k], 1.0, L[s]);
    }
#pragma unroll
    for (int m = 0; m < 10; ++m) {
      const double h = 0.5 * (L[0][m] + L[3][m] + L[5][m]);
      L[0][m] -= h, L[3][m] -= h, L[5][m] -= h;
    }
    const int sym[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        double acc[20];
#pragma unroll
        for (int m = 0; m < 20; ++m) acc[m] = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) es_mul21(L[sym[r][k]], El[k * 3 + c], acc);
        double ss = 0.0;
#pragma unroll
        for (int m = 0; m < 20; ++m) ss += acc[m] * acc[m];
        const double nrm = sqrt(ss);
#pragma unroll
        for (int m = 0; m < 20; ++m) M_(r * 3 + c, m) = acc[m] / nrm;
      }
    double acc[20];
#pragma unroll
    for (int m = 0; m < 20; ++m) acc[m] = 0.0;
    const int ca[3] = {1, 0, 0}, cb[3] = {2, 2, 1};   // the minors of row 0: columns (1,2), (0,2), (0,1) of rows 1 and 2
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double mn[10];
#pragma unroll
      for (int m = 0; m < 10; ++m) mn[m] = 0.0;
      const double sg = c == 1 ? -1.0 : 1.0;
      es_mul11(El[3 + ca[c]], El[6 + cb[c]], sg, mn);
      es_mul11(El[3 + cb[c]], El[6 + ca[c]], -sg, mn);
      es_mul21(mn, El[c], acc);
    }
    double ss = 0.0;
#pragma unroll
    for (int m = 0; m < 20; ++m) ss += acc[m] * acc[m];
    const double nrm = sqrt(ss);
#pragma unroll
    for (int m = 0; m < 20; ++m) M_(9, m) = acc[m] / nrm;
  }
  // 3. Gauss-Jordan elimination of the ten cubic monomials with row pivoting: [I | B]
  double piv0 = 0.0;
  for (int k = 0; k < 10; ++k) {
    double pv = -1.0;
    int pr = k;
    for (int r = k; r < 10; ++r) {
      const double v = fabs(M_(r, k));
      if (v > pv) pv = v, pr = r;
    }
    if (k == 0) piv0 = pv;
    if (!(pv > RS_RANK_TOL * piv0)) return 0;   // also for NaN
    if (pr != k)
      for (int c = k; c < 20; ++c) {
        const double t = M_(k, c);
        M_(k, c) = M_(pr, c);
        M_(pr, c) = t;
      }
    const double akk = M_(k, k);
    for (int c = k + 1; c < 20; ++c) M_(k, c) = M_(k, c) / akk;
    M_(k, k) = 1.0;
    double prow[20];   // the pivot row and each row through registers, so that their LDS reads are in flight together
#pragma unroll
    for (int c = 0; c < 20; ++c) prow[c] = M_(k, c);
    for (int r = 0; r < 10; ++r) {
      if (r == k) continue;
      const double m = M_(r, k);
      double row[20];
#pragma unroll
      for (int c = 0; c < 20; ++c) row[c] = M_(r, c);
#pragma unroll
      for (int c = 0; c < 20; ++c) M_(r, c) = c > k ? row[c] - m * prow[c] : (c == k ? 0.0 : row[c]);
    }
  }
  // 4. the real eigenvalues of the action matrix are the x of the real solutions, ascending
  es_action<STRIDE>(mem, 0.0);
  const int nreal = es_real_eigenvalues<STRIDE>(mem);
  if (nreal <= 0) return 0;
  for (int i = 1; i < nreal; ++i) {
    const double v = WR_(i);
    int j = i - 1;
    for (; j >= 0 && WR_(j) > v; --j) WR_(j + 1) = WR_(j);
    WR_(j + 1) = v;
  }
  // 5. every root: its eigenvector (the null vector of A - x I by full-pivot elimination) gives y and z; polish; the candidate
  for (int k = 0; k < nreal; ++k) {
    double p[3] = {WR_(k), NAN, NAN};
    es_action<STRIDE>(mem, p[0]);
    for (int c = 0; c < 10; ++c) P_(c) = c;
    bool ok = true;
    for (int s = 0; s < 9 && ok; ++s) {
      double pv = -1.0;
      int pr = s, pc = s;
      for (int r = s; r < 10; ++r)
        for (int c = s; c < 10; ++c) {
          const double v = fabs(M_(r, c));
          if (v > pv) pv = v, pr = r, pc = c;
        }
      if (!(pv > 0.0)) {   // also for NaN
        ok = false;
        break;
      }
      if (pr != s)
        for (int c = 0; c < 10; ++c) {
          const double t = M_(s, c);
          M_(s, c) = M_(pr, c);
          M_(pr, c) = t;
        }
      if (pc != s) {
        for (int r = 0; r < 10; ++r) {
          const double t = M_(r, s);
          M_(r, s) = M_(r, pc);
          M_(r, pc) = t;
        }
        const int t = P_(s);
        P_(s) = P_(pc);
        P_(pc) = t;
      }
      const double akk = M_(s, s);
      double prow[10];
#pragma unroll
      for (int c = 0; c < 10; ++c) prow[c] = M_(s, c);
      for (int r = s + 1; r < 10; ++r) {
        const double m = M_(r, s) / akk;
        double row[10];
#pragma unroll
        for (int c = 0; c < 10; ++c) row[c] = M_(r, c);
#pragma unroll
        for (int c = 0; c < 10; ++c) M_(r, c) = c > s ? row[c] - m * prow[c] : (c == s ? 0.0 : row[c]);
      }
    }
    if (ok) {
      T_(9) = 1.0;
      for (int r = 8; r >= 0; --r) {
        double acc = 0.0;
        for (int c = r + 1; c < 10; ++c) acc += M_(r, c) * T_(c);
        T_(r) = -acc / M_(r, r);
      }
      double vy = NAN, vz = NAN, vw = NAN;
      for (int c = 0; c < 10; ++c) {
        const int o = P_(c);
        const double v = T_(c);
        vy = o == 7 ? v : vy, vz = o == 8 ? v : vz, vw = o == 9 ? v : vw;
      }
      p[1] = vy / vw, p[2] = vz / vw;
      for (int s = 0; s < ES_POLISH; ++s) es_polish_step<STRIDE>(mem, perm, p);
    }
    double E[9], ss = 0.0;
#pragma unroll
    for (int e = 0; e < 9; ++e) {
      E[e] = p[0] * El[e][0] + p[1] * El[e][1] + p[2] * El[e][2] + El[e][3];
      ss += E[e] * E[e];
    }
    const double nrm = sqrt(ss);
#pragma unroll
    for (int e = 0; e < 9; ++e) E[e] = E[e] / nrm;
    const bool negative = rs_negative9(E);
#pragma unroll
    for (int e = 0; e < 9; ++e) out[k * 9 + e] = negative ? -E[e] : E[e];
  }
  return nreal;
}
#undef M_
#undef Q_
#undef NS_
#undef WR_
#undef T_
#undef P_

// ---- points and errors ----------------------------------------------------------------------------------------------
// (EsCam and es_normalise, the pixel -> normalised coordinates rule: pinhole.h)
// Sampson error of the normalised pair (x1, y1) -> (x2, y2)
ES_HD __forceinline__ float es_error(const double* e, double x1, double y1, double x2, double y2) {
  const double a0 = e[0] * x1 + e[1] * y1 + e[2], a1 = e[3] * x1 + e[4] * y1 + e[5], a2 = e[6] * x1 + e[7] * y1 + e[8];
  const double b0 = e[0] * x2 + e[3] * y2 + e[6], b1 = e[1] * x2 + e[4] * y2 + e[7];
  const double d = x2 * a0 + y2 * a1 + a2;
  return (float)(d * d / (a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1));
}

// the model of ransac.h's frame: up to 10 candidates per 5-point sample, on the normalised pairs xn [n, 4]; the tail zeroes
// info[4..7]
struct EsModel {
  static constexpr int MODEL = ES_MODEL, SLOTS = ES_SLOTS;
  struct Points {
    const double* __restrict__ xn;
  };
  struct Tail {
    int32_t* info_tail;
  };

  static __device__ __forceinline__ bool inlier(const double* e, const Points& pts, int p, float thr) {
    const double* q = pts.xn + (size_t)p * 4;
    return es_error(e, q[0], q[1], q[2], q[3]) <= thr;   // false for NaN
  }

  static __device__ __forceinline__ void tail(const Tail& t, int) {
    for (int i = 0; i < 4; ++i) t.info_tail[i] = 0;
  }
};

// The least-squares depths (z1, z2) of z2 x2h = z1 a + t, a = R x1h, for t and for -t: in front iff both lie in (0, dist).
// bit 0: (R, t), bit 1: (R, -t).  A zero determinant: in front of neither.
ES_HD __forceinline__ int es_in_front(const double* R, const double* t, double x1, double y1, double x2, double y2, double dist) {
  const double a0 = R[0] * x1 + R[1] * y1 + R[2], a1 = R[3] * x1 + R[4] * y1 + R[5], a2 = R[6] * x1 + R[7] * y1 + R[8];
  const double aa = a0 * a0 + a1 * a1 + a2 * a2, ab = a0 * x2 + a1 * y2 + a2, bb = x2 * x2 + y2 * y2 + 1.0;
  const double at = a0 * t[0] + a1 * t[1] + a2 * t[2], bt = x2 * t[0] + y2 * t[1] + t[2];
  const double det = aa * bb - ab * ab;
  if (det == 0.0) return 0;
  const double z1 = (ab * bt - at * bb) / det, z2 = (aa * bt - ab * at) / det;
  const int plus = (z1 > 0.0 && z1 < dist && z2 > 0.0 && z2 < dist) ? 1 : 0;
  const int minus = (-z1 > 0.0 && -z1 < dist && -z2 > 0.0 && -z2 < dist) ? 2 : 0;
  return plus | minus;
}

// ---- kernels of cotr_ransac_essential -----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void es_normalise_kernel(const double* __restrict__ pts1, const double* __restrict__ pts2, int n, EsCam k1,
                                                           EsCam k2, double* __restrict__ xn) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  double x1, y1, x2, y2;
  es_normalise(k1, pts1[(size_t)p * 2], pts1[(size_t)p * 2 + 1], &x1, &y1);
  es_normalise(k2, pts2[(size_t)p * 2], pts2[(size_t)p * 2 + 1], &x2, &y2);
  double* q = xn + (size_t)p * 4;
  q[0] = x1, q[1] = y1, q[2] = x2, q[3] = y2;
}

__global__ __launch_bounds__(ES_SOLVE_THREADS) void es_solve_kernel(const double* __restrict__ xn, int n, int max_iters, uint64_t seed,
                                                                    double* __restrict__ Ec, int* __restrict__ count,
                                                                    double* __restrict__ hyp_E, int32_t* __restrict__ hyp_samples) {
  // per-thread LDS columns: sh[e * 32 + lane] (the eliminations and the QR iteration index rows and columns at run time)
  __shared__ double shD[ES_DOUBLES * ES_SOLVE_THREADS];
  __shared__ int shI[ES_INTS * ES_SOLVE_THREADS];
  const int lane = threadIdx.x;
  const int it = blockIdx.x * ES_SOLVE_THREADS + lane;
  if (it >= max_iters) return;   // no workgroup barrier below
#define S_(k) shI[(k) * ES_SOLVE_THREADS + lane]
  const int got = rs_sample<ES_MODEL>(seed, it, n, &shI[lane], ES_SOLVE_THREADS);
  if (hyp_samples) {
    for (int k = 0; k < ES_MODEL; ++k) hyp_samples[(size_t)it * ES_MODEL + k] = k < got ? S_(k) : -1;
  }
  double* out = Ec + (size_t)it * ES_SLOTS * 9;
  int nc = 0;
  if (got == ES_MODEL) {
    double x1[ES_MODEL], y1[ES_MODEL], x2[ES_MODEL], y2[ES_MODEL];
#pragma unroll
    for (int k = 0; k < ES_MODEL; ++k) {
      const double* q = xn + (size_t)S_(k) * 4;
      x1[k] = q[0], y1[k] = q[1], x2[k] = q[2], y2[k] = q[3];
    }
    nc = es_five_point<ES_SOLVE_THREADS>(x1, y1, x2, y2, &shD[lane], &shI[ES_MODEL * ES_SOLVE_THREADS + lane], out);
  }
#undef S_
  // the slots 10 * it + k: a candidate counts from 0; a slot without one is NaN with count -1
  for (int k = 0; k < ES_SLOTS; ++k) {
    const size_t slot = (size_t)it * ES_SLOTS + k;
    if (k >= nc)
      for (int i = 0; i < 9; ++i) out[k * 9 + i] = NAN;
    if (hyp_E)
      for (int i = 0; i < 9; ++i) hyp_E[slot * 9 + i] = out[k * 9 + i];
    count[slot] = k < nc ? 0 : -1;
  }
}

// ---- kernels of cotr_recover_pose ---------------------------------------------------------------------------------------
// in scratch: the two rotations, t, whether E could be decomposed, the four counts
struct EsPose {
  double R[2][9];
  double t[3];
  int valid;
  int counts[4];
};

__global__ __launch_bounds__(64) void es_decompose_kernel(const double* __restrict__ E, const int32_t* __restrict__ found, EsPose* __restrict__ st) {
  __shared__ double A[3][3], V[3][3];
  if (threadIdx.x != 0) return;
  double e[9];
  bool ok = found == nullptr || found[0] != 0;
  for (int i = 0; i < 9; ++i) {
    e[i] = E[i];
    ok = ok && isfinite(e[i]);
  }
  double U[3][3] = {}, Vm[3][3] = {};
  if (ok) {
    // V: the eigenvectors of E^T E by cyclic Jacobi; column m of the smallest eigenvalue goes last, the other two keep their order
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) A[i][j] = e[i] * e[j] + e[3 + i] * e[3 + j] + e[6 + i] * e[6 + j];
    rs_jacobi<3>(A, V);
    int m = 0;
    for (int i = 1; i < 3; ++i)
      if (A[i][i] < A[m][m]) m = i;
    const int c0 = m == 0 ? 1 : 0, c1 = m == 2 ? 1 : 2;
    for (int i = 0; i < 3; ++i) Vm[i][0] = V[i][c0], Vm[i][1] = V[i][c1], Vm[i][2] = V[i][m];
    // U: E v / sigma for the two leading columns, their cross product for the third
    for (int c = 0; c < 2; ++c) {
      double u[3], ss = 0.0;
      for (int i = 0; i < 3; ++i) {
        u[i] = e[i * 3] * Vm[0][c] + e[i * 3 + 1] * Vm[1][c] + e[i * 3 + 2] * Vm[2][c];
        ss += u[i] * u[i];
      }
      const double sg = sqrt(ss);
      ok = ok && sg > 0.0;
      for (int i = 0; i < 3; ++i) U[i][c] = u[i] / sg;
    }
    U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
    U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
    U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
    // det U = 1 by construction; det V > 0 by the sign of its last column
    const double dv = Vm[0][0] * (Vm[1][1] * Vm[2][2] - Vm[1][2] * Vm[2][1]) - Vm[0][1] * (Vm[1][0] * Vm[2][2] - Vm[1][2] * Vm[2][0]) +
                      Vm[0][2] * (Vm[1][0] * Vm[2][1] - Vm[1][1] * Vm[2][0]);
    if (dv < 0.0)
      for (int i = 0; i < 3; ++i) Vm[i][2] = -Vm[i][2];
  }
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) {
      // R1 = U W V^T and R2 = U W^T V^T with W = [0 1 0; -1 0 0; 0 0 1]: U W = [-u1, u0, u2], U W^T = [u1, -u0, u2]
      const double r1 = -U[i][1] * Vm[j][0] + U[i][0] * Vm[j][1] + U[i][2] * Vm[j][2];
      const double r2 = U[i][1] * Vm[j][0] - U[i][0] * Vm[j][1] + U[i][2] * Vm[j][2];
      st->R[0][i * 3 + j] = ok ? r1 : 0.0;
      st->R[1][i * 3 + j] = ok ? r2 : 0.0;
    }
    st->t[i] = ok ? U[i][2] : 0.0;
  }
  st->valid = ok ? 1 : 0;
  for (int c = 0; c < 4; ++c) st->counts[c] = 0;
}

// bits 0..3 of a point: in front of (R1, t), (R2, t), (R1, -t), (R2, -t)
__device__ __forceinline__ int es_front_bits(const EsPose* __restrict__ st, const EsCam& k1, const EsCam& k2, const double* __restrict__ pts1,
                                             const double* __restrict__ pts2, int p, double dist) {
  double x1, y1, x2, y2;
  es_normalise(k1, pts1[(size_t)p * 2], pts1[(size_t)p * 2 + 1], &x1, &y1);
  es_normalise(k2, pts2[(size_t)p * 2], pts2[(size_t)p * 2 + 1], &x2, &y2);
  const int f1 = es_in_front(st->R[0], st->t, x1, y1, x2, y2, dist), f2 = es_in_front(st->R[1], st->t, x1, y1, x2, y2, dist);
  return (f1 & 1) | ((f2 & 1) << 1) | ((f1 & 2) << 1) | ((f2 & 2) << 2);
}

__global__ __launch_bounds__(RS_COUNT_THREADS) void es_front_kernel(const double* __restrict__ pts1, const double* __restrict__ pts2, int n,
                                                                    EsCam k1, EsCam k2, const uint8_t* __restrict__ mask, double dist,
                                                                    EsPose* __restrict__ st) {
  if (!st->valid) return;   // uniform
  const int base = blockIdx.x * RS_CHUNK;
  int wc[4] = {0, 0, 0, 0};
#pragma unroll 1
  for (int s = 0; s < RS_COUNT_STEPS; ++s) {
    const int p = base + s * RS_COUNT_THREADS + threadIdx.x;
    const int bits = (p < n && (mask == nullptr || mask[p])) ? es_front_bits(st, k1, k2, pts1, pts2, p, dist) : 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) wc[c] += __popcll(__ballot((bits >> c) & 1));
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (wc[c] > 0) atomicAdd(&st->counts[c], wc[c]);
  }
}

__global__ __launch_bounds__(256) void es_pose_kernel(const double* __restrict__ pts1, const double* __restrict__ pts2, int n, EsCam k1, EsCam k2,
                                                      const uint8_t* __restrict__ mask, double dist, const EsPose* __restrict__ st,
                                                      double* __restrict__ R_out, double* __restrict__ t_out, uint8_t* __restrict__ mask_out,
                                                      int32_t* __restrict__ info) {
  const int valid = st->valid;
  int chosen = 0;   // the first candidate with the largest count
  for (int c = 1; c < 4; ++c)
    if (st->counts[c] > st->counts[chosen]) chosen = c;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p < n) {
    const int bits = (valid && (mask == nullptr || mask[p])) ? es_front_bits(st, k1, k2, pts1, pts2, p, dist) : 0;
    mask_out[p] = (bits >> chosen) & 1;
  }
  if (p < 9) R_out[p] = valid ? st->R[chosen & 1][p] : 0.0;
  if (p < 3) t_out[p] = valid ? (chosen >= 2 ? -st->t[p] : st->t[p]) : 0.0;
  if (p == 0) {
    info[0] = valid ? st->counts[chosen] : 0;
    info[1] = valid ? chosen : -1;
    for (int c = 0; c < 4; ++c) info[2 + c] = valid ? st->counts[c] : 0;
    info[6] = 0;
    info[7] = 0;
  }
}

// ---- kernels of cotr_refine_pose ----------------------------------------------------------------------------------------
#define RP_PARAMS 5            // w (3) of R <- exp([w]x) R, then (u, v) of t <- (t + u b1 + v b2) / |...|
#define RP_SUMS 22             // 15 of J^T J, 5 of J^T r, the squared error, the points skipped
#define RP_MAX_ROUNDS 8
#define RP_MAX_REFINE 64

struct RpState;
__device__ void rp_derive(RpState* __restrict__ st);

// in scratch (the pose: |t| = 1; done, kept: of this round), and the model of refit.h's step
struct RpState : RfPose {
  double E[9];                 // [t]x R
  double dE[RP_PARAMS][9];     // its derivative in the five directions
  double b1[3], b2[3];         // the tangent basis at t
  int valid;                   // found, and R_in, t_in finite with t_in != 0
  int kept_total, kept_last, rounds_run, skipped;
  int count[RP_MAX_ROUNDS];    // points in each round's mask

  static constexpr int PARAMS = RP_PARAMS;
  static __device__ __forceinline__ bool solvable(const RpState* st, int round) { return st->count[round] >= ES_MODEL; }
  static __device__ __forceinline__ void evaluated(RpState* st, const double* sums) { st->skipped = (int)sums[21]; }
  static __device__ __forceinline__ void restore(RpState* st) {
    RfPose::restore(st);
    rp_derive(st);
  }
  static __device__ __forceinline__ void apply(RpState* st, const double* d) {
    rotate(st, d);
    const double x = (st->t[0] + d[3] * st->b1[0]) + d[4] * st->b2[0], y = (st->t[1] + d[3] * st->b1[1]) + d[4] * st->b2[1],
                 z = (st->t[2] + d[3] * st->b1[2]) + d[4] * st->b2[2];
    const double nrm = sqrt((x * x + y * y) + z * z);
    st->t[0] = x / nrm, st->t[1] = y / nrm, st->t[2] = z / nrm;
    rp_derive(st);
  }
};

// out = [v]x M
__device__ __forceinline__ void rp_cross(const double* v, const double* M, double* out) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    out[c] = v[1] * M[6 + c] - v[2] * M[3 + c];
    out[3 + c] = v[2] * M[c] - v[0] * M[6 + c];
    out[6 + c] = v[0] * M[3 + c] - v[1] * M[c];
  }
}

// From R and t of st: the tangent basis (k: the first index of smallest |t_k|; b1 = e_k x t normalised, b2 = t x b1),
// E = [t]x R and dE = [t]x [e_j]x R for j = 0..2, [b1]x R, [b2]x R.  One thread.
__device__ void rp_derive(RpState* __restrict__ st) {
  double R[9], t[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = st->R[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = st->t[i];
  const double m0 = fabs(t[0]), m1 = fabs(t[1]), m2 = fabs(t[2]);
  const int k = (m0 <= m1 && m0 <= m2) ? 0 : (m1 <= m2 ? 1 : 2);
  const double c[3] = {k == 0 ? 0.0 : (k == 1 ? t[2] : -t[1]), k == 0 ? -t[2] : (k == 1 ? 0.0 : t[0]),
                       k == 0 ? t[1] : (k == 1 ? -t[0] : 0.0)};
  const double nrm = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
  const double b1[3] = {c[0] / nrm, c[1] / nrm, c[2] / nrm};
  const double b2[3] = {t[1] * b1[2] - t[2] * b1[1], t[2] * b1[0] - t[0] * b1[2], t[0] * b1[1] - t[1] * b1[0]};
#pragma unroll
  for (int i = 0; i < 3; ++i) st->b1[i] = b1[i], st->b2[i] = b2[i];
  double out[9];
  rp_cross(t, R, out);
#pragma unroll
  for (int i = 0; i < 9; ++i) st->E[i] = out[i];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double e[3] = {j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0};
    double M[9];
    rp_cross(e, R, M);
    rp_cross(t, M, out);
#pragma unroll
    for (int i = 0; i < 9; ++i) st->dE[j][i] = out[i];
  }
  rp_cross(b1, R, out);
#pragma unroll
  for (int i = 0; i < 9; ++i) st->dE[3][i] = out[i];
  rp_cross(b2, R, out);
#pragma unroll
  for (int i = 0; i < 9; ++i) st->dE[4][i] = out[i];
}

__global__ __launch_bounds__(64) void rp_init_kernel(const double* __restrict__ R_in, const double* __restrict__ t_in,
                                                     const int32_t* __restrict__ found, RpState* __restrict__ st) {
  if (threadIdx.x != 0) return;
  bool ok = found == nullptr || found[0] != 0;
  double R[9], t[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    R[i] = R_in[i];
    ok = ok && isfinite(R[i]);
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    t[i] = t_in[i];
    ok = ok && isfinite(t[i]);
  }
  const double nrm = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
  ok = ok && nrm > 0.0 && nrm < INFINITY;
#pragma unroll
  for (int i = 0; i < 9; ++i) st->R[i] = ok ? R[i] : 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) st->t[i] = ok ? t[i] / nrm : 0.0;
  st->valid = ok ? 1 : 0;
  st->done = ok ? 0 : 1;
  st->trial = 0;
  st->kept = 0, st->kept_total = 0, st->kept_last = 0, st->rounds_run = 0, st->skipped = 0;
  for (int r = 0; r < RP_MAX_ROUNDS; ++r) st->count[r] = 0;
  if (ok) {
    rp_derive(st);
  } else {
#pragma unroll
    for (int i = 0; i < 9; ++i) st->E[i] = 0.0;
  }
}

// The round's mask and its count.  first: the caller's mask (NULL: every point); later rounds: the Sampson inliers of the
// current E that lie in front of both cameras under the current (R, t).
__global__ __launch_bounds__(RS_COUNT_THREADS) void rp_mask_kernel(const double* __restrict__ xn, int n, const uint8_t* __restrict__ mask_in,
                                                                   int first, float thr, double dist, int round, RpState* __restrict__ st,
                                                                   uint8_t* __restrict__ mask_out) {
  const int valid = st->valid;   // uniform
  double E[9], R[9], t[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) E[i] = st->E[i], R[i] = st->R[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = st->t[i];
  const int base = blockIdx.x * RS_CHUNK;
  int wc = 0;
#pragma unroll 1
  for (int s = 0; s < RS_COUNT_STEPS; ++s) {
    const int p = base + s * RS_COUNT_THREADS + threadIdx.x;
    bool in = false;
    if (p < n && valid) {
      if (first) {
        in = mask_in == nullptr || mask_in[p] != 0;
      } else {
        const double* q = xn + (size_t)p * 4;
        in = EsModel::inlier(E, {xn}, p, thr) && (es_in_front(R, t, q[0], q[1], q[2], q[3], dist) & 1) != 0;
      }
    }
    if (p < n) mask_out[p] = in ? 1 : 0;
    wc += __popcll(__ballot(in));
  }
  if ((threadIdx.x & 63) == 0 && wc > 0) atomicAdd(&st->count[round], wc);
}

// One masked point's terms at the state st, added to acc: J^T J (15), J^T r (5), r^2; a point with g = 0 or a residual that is
// not finite adds 1 to acc[21] and nothing else.  r = d / sqrt(g) with a = E x1h, b = E^T x2h, d = x2h . a,
// g = a0^2 + a1^2 + b0^2 + b1^2; its derivative by the quotient rule.
__device__ __forceinline__ void rp_terms(const RpState* __restrict__ st, double x1, double y1, double x2, double y2, double* acc) {
  const double* e = st->E;
  const double a0 = e[0] * x1 + e[1] * y1 + e[2], a1 = e[3] * x1 + e[4] * y1 + e[5], a2 = e[6] * x1 + e[7] * y1 + e[8];
  const double b0 = e[0] * x2 + e[3] * y2 + e[6], b1 = e[1] * x2 + e[4] * y2 + e[7];
  const double d = x2 * a0 + y2 * a1 + a2;
  const double g = a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1;
  const double s = sqrt(g), r = d / s;
  if (!(g > 0.0) || !isfinite(r)) {
    acc[21] += 1.0;
    return;
  }
  double J[RP_PARAMS];
#pragma unroll
  for (int k = 0; k < RP_PARAMS; ++k) {
    const double* q = st->dE[k];
    const double da0 = q[0] * x1 + q[1] * y1 + q[2], da1 = q[3] * x1 + q[4] * y1 + q[5], da2 = q[6] * x1 + q[7] * y1 + q[8];
    const double db0 = q[0] * x2 + q[3] * y2 + q[6], db1 = q[1] * x2 + q[4] * y2 + q[7];
    const double dd = x2 * da0 + y2 * da1 + da2;
    const double dg = 2.0 * (a0 * da0 + a1 * da1 + b0 * db0 + b1 * db1);
    J[k] = dd / s - d * dg / (2.0 * s * g);
  }
#pragma unroll
  for (int i = 0; i < RP_PARAMS; ++i) {
#pragma unroll
    for (int j = i; j < RP_PARAMS; ++j) acc[rf_tri<RP_PARAMS>(i, j)] += J[i] * J[j];
    acc[15 + i] += J[i] * r;
  }
  acc[20] += r * r;
}

struct RpTerms {
  static constexpr int SUMS = RP_SUMS, STRIDE = RP_SUMS;
  using Points = EsModel::Points;
  using State = RpState;
  static __device__ __forceinline__ void terms(const RpState* __restrict__ st, const Points& pts, int p, double* acc) {
    const double* q = pts.xn + (size_t)p * 4;
    rp_terms(st, q[0], q[1], q[2], q[3], acc);
  }
};

// the sums of the accumulate before it: judges the step on trial, takes the next one (fewer than 5 points in the round's mask:
// none);
// last: the round's last launch (no further step is taken; the state is made ready for the next round);
// final: the call's last launch (writes R_out, t_out, E_out and info)
__global__ __launch_bounds__(64) void rp_finish_kernel(int chunks, const double* __restrict__ parts, RpState* __restrict__ st, int round,
                                                       int last, int final, double* __restrict__ R_out, double* __restrict__ t_out,
                                                       double* __restrict__ E_out, int32_t* __restrict__ info) {
  __shared__ double sums[RP_SUMS];
  const bool active = !st->done;   // uniform; read before anything below writes it
  rf_reduce<RP_SUMS>(parts, chunks, active ? RP_SUMS : 0, sums);
  if (threadIdx.x != 0) return;
  const int valid = st->valid;
  if (active) rf_step(st, sums, last, round);
  if (last && valid) {   // the round is over: its steps counted, the flag lowered for the next one
    st->kept_total = st->kept_total + st->kept;
    st->kept_last = st->kept;
    st->rounds_run = st->rounds_run + 1;
    st->kept = 0;
    st->trial = 0;
    st->done = 0;
  }
  if (final) {
    double e[9], ss = 0.0;
    for (int i = 0; i < 9; ++i) {
      e[i] = st->E[i];
      ss += e[i] * e[i];
    }
    const double nrm = sqrt(ss);
    for (int i = 0; i < 9; ++i) e[i] = e[i] / nrm;
    const bool negative = rs_negative9(e);
    for (int i = 0; i < 9; ++i) {
      R_out[i] = valid ? st->R[i] : 0.0;
      E_out[i] = valid ? (negative ? -e[i] : e[i]) : 0.0;
    }
    for (int i = 0; i < 3; ++i) t_out[i] = valid ? st->t[i] : 0.0;
    info[0] = valid;
    info[1] = st->count[round];
    info[2] = st->rounds_run;
    info[3] = st->kept_total;
    info[4] = st->kept_last;
    info[5] = st->skipped;
    info[6] = 0;
    info[7] = 0;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
namespace {

const RsEntry ES_ENTRY = {"cotr_ransac_essential", "E_out", ES_MODEL, "", ES_SLOTS, ES_MAX_ITERS};

// after the frame's candidates and counts: the normalised pairs xn [n, 4]
size_t es_scratch_bytes(const RsPlan& l, int n) { return l.bytes + align_up((size_t)n * 4 * sizeof(double)); }

// the scratch of cotr_refine_pose: the normalised pairs xn [n, 4], the state, the partial sums [chunks, RP_SUMS]
RfPlan rp_plan(int n) { return rf_plan(align_up((size_t)n * 4 * sizeof(double)), sizeof(RpState), n, RP_SUMS); }

}  // namespace

extern "C" {

int cotr_ransac_essential_scratch_bytes(int n, int max_iters, size_t* bytes) {
  if (const int rc = rs_scratch_bytes(ES_ENTRY, n, max_iters, bytes)) return rc;
  *bytes = es_scratch_bytes(rs_plan(ES_ENTRY, max_iters), n);
  return COTR_OK;
}

int cotr_ransac_essential(const double* pts1, const double* pts2, int n, const double* K1, const double* K2, double threshold,
                          double confidence, int max_iters, uint64_t seed, double* E_out, uint8_t* mask_out, int32_t* info_out,
                          double* hyp_E, int32_t* hyp_count, int32_t* hyp_samples, void* scratch, size_t scratch_bytes, cotr_stream stream) {
  const RsPlan l = rs_plan(ES_ENTRY, max_iters);
  if (const int rc = rs_check_call(ES_ENTRY, n, max_iters, threshold, confidence, pts1, pts2, E_out, mask_out, info_out, hyp_E, hyp_count,
                                   hyp_samples, scratch, scratch_bytes, es_scratch_bytes(l, n)))
    return rc;
  if (!K1 || !K2) return rs_fail(ES_ENTRY, "K1 and K2 must not be NULL");
  EsCam k1, k2;
  if (!es_camera(K1, &k1) || !es_camera(K2, &k2)) return rs_fail(ES_ENTRY, "the camera matrices must be finite with focal lengths that are not 0");
  const double focal = (k1.fx + k1.fy + k2.fx + k2.fy) / 4.0;
  const double thr = threshold / focal;
  if (!(thr * thr > 0.0) || !(thr * thr < INFINITY))
    return rs_fail(ES_ENTRY, "the threshold over the mean focal length must be finite and not 0");
  double* xn = reinterpret_cast<double*>(static_cast<char*>(scratch) + l.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(es_normalise_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pts1, pts2, n, k1, k2, xn);
  const auto solve = [&](double* Ec, int* count) {
    hipLaunchKernelGGL(es_solve_kernel, dim3((unsigned)((max_iters + ES_SOLVE_THREADS - 1) / ES_SOLVE_THREADS)), dim3(ES_SOLVE_THREADS), 0, s, xn, n,
                       max_iters, seed, Ec, count, hyp_E, hyp_samples);
  };
  rs_enqueue<EsModel>(s, solve, {xn}, n, max_iters, confidence, (float)(thr * thr), l, scratch, E_out, mask_out, info_out, hyp_count,
                      {info_out + 4});
  return launched();
}

int cotr_recover_pose_scratch_bytes(int n, size_t* bytes) {
  if (!bytes) return handleless_fail(COTR_ERR_ARG, "cotr_recover_pose_scratch_bytes: bytes is NULL");
  if (n < ES_MODEL || n > RS_MAX_POINTS) return handleless_fail(COTR_ERR_ARG, "cotr_recover_pose: n must be in [5, 2^24]");
  *bytes = align_up(sizeof(EsPose));
  return COTR_OK;
}

int cotr_recover_pose(const double* E, const double* pts1, const double* pts2, int n, const double* K1, const double* K2, double distance_thresh,
                      const uint8_t* mask_in, const int32_t* found, double* R_out, double* t_out, uint8_t* mask_out, int32_t* info_out,
                      void* scratch, size_t scratch_bytes, cotr_stream stream) {
  if (n < ES_MODEL || n > RS_MAX_POINTS) return handleless_fail(COTR_ERR_ARG, "cotr_recover_pose: n must be in [5, 2^24]");
  if (!(distance_thresh > 0.0) || !(distance_thresh < INFINITY))
    return handleless_fail(COTR_ERR_ARG, "cotr_recover_pose: distance_thresh must be finite and > 0");
  if (!E || !pts1 || !pts2 || !K1 || !K2 || !R_out || !t_out || !mask_out || !info_out || !scratch)
    return handleless_fail(COTR_ERR_ARG, "cotr_recover_pose: E, pts1, pts2, K1, K2, R_out, t_out, mask_out, info_out and scratch must not be NULL");
  EsCam k1, k2;
  if (!es_camera(K1, &k1) || !es_camera(K2, &k2))
    return handleless_fail(COTR_ERR_ARG, "cotr_recover_pose: the camera matrices must be finite with focal lengths that are not 0");
  if (!aligned(E, 8) || !aligned(pts1, 8) || !aligned(pts2, 8) || !aligned(R_out, 8) || !aligned(t_out, 8) || !aligned(info_out, 4) ||
      !aligned(found, 4) || !aligned(scratch, 16))
    return handleless_fail(COTR_ERR_ARG, "cotr_recover_pose: doubles must be 8-byte, ints 4-byte and scratch 16-byte aligned");
  if (scratch_bytes < align_up(sizeof(EsPose))) return handleless_fail(COTR_ERR_ARG, "cotr_recover_pose: scratch is smaller than cotr_recover_pose_scratch_bytes");
  EsPose* st = static_cast<EsPose*>(scratch);
  const int chunks = (n + RS_CHUNK - 1) / RS_CHUNK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(es_decompose_kernel, dim3(1), dim3(64), 0, s, E, found, st);
  hipLaunchKernelGGL(es_front_kernel, dim3((unsigned)chunks), dim3(RS_COUNT_THREADS), 0, s, pts1, pts2, n, k1, k2, mask_in, distance_thresh, st);
  hipLaunchKernelGGL(es_pose_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pts1, pts2, n, k1, k2, mask_in, distance_thresh, st, R_out,
                     t_out, mask_out, info_out);
  return launched();
}

int cotr_refine_pose_scratch_bytes(int n, size_t* bytes) {
  if (!bytes) return handleless_fail(COTR_ERR_ARG, "cotr_refine_pose_scratch_bytes: bytes is NULL");
  if (n < ES_MODEL || n > RS_MAX_POINTS) return handleless_fail(COTR_ERR_ARG, "cotr_refine_pose: n must be in [5, 2^24]");
  *bytes = rp_plan(n).bytes;
  return COTR_OK;
}

int cotr_refine_pose(const double* R_in, const double* t_in, const double* pts1, const double* pts2, int n, const double* K1, const double* K2,
                     double threshold, double distance_thresh, int rounds, int refine_iters, const uint8_t* mask_in, const int32_t* found,
                     double* R_out, double* t_out, double* E_out, uint8_t* mask_out, int32_t* info_out, void* scratch, size_t scratch_bytes,
                     cotr_stream stream) {
  if (n < ES_MODEL || n > RS_MAX_POINTS) return handleless_fail(COTR_ERR_ARG, "cotr_refine_pose: n must be in [5, 2^24]");
  if (!(threshold > 0.0) || !(threshold < INFINITY)) return handleless_fail(COTR_ERR_ARG, "cotr_refine_pose: threshold must be finite and > 0");
  if (!(distance_thresh > 0.0) || !(distance_thresh < INFINITY))
    return handleless_fail(COTR_ERR_ARG, "cotr_refine_pose: distance_thresh must be finite and > 0");
  if (rounds < 1 || rounds > RP_MAX_ROUNDS) return handleless_fail(COTR_ERR_ARG, "cotr_refine_pose: rounds must be in [1, 8]");
  if (refine_iters < 0 || refine_iters > RP_MAX_REFINE) return handleless_fail(COTR_ERR_ARG, "cotr_refine_pose: refine_iters must be in [0, 64]");
  if (!R_in || !t_in || !pts1 || !pts2 || !K1 || !K2 || !R_out || !t_out || !E_out || !mask_out || !info_out || !scratch)
    return handleless_fail(COTR_ERR_ARG,
                           "cotr_refine_pose: R_in, t_in, pts1, pts2, K1, K2, R_out, t_out, E_out, mask_out, info_out and scratch must not be NULL");
  EsCam k1, k2;
  if (!es_camera(K1, &k1) || !es_camera(K2, &k2))
    return handleless_fail(COTR_ERR_ARG, "cotr_refine_pose: the camera matrices must be finite with focal lengths that are not 0");
  const double focal = (k1.fx + k1.fy + k2.fx + k2.fy) / 4.0;
  const double thr = threshold / focal;
  if (!(thr * thr > 0.0) || !(thr * thr < INFINITY))
    return handleless_fail(COTR_ERR_ARG, "cotr_refine_pose: the threshold over the mean focal length must be finite and not 0");
  if (!aligned(R_in, 8) || !aligned(t_in, 8) || !aligned(pts1, 8) || !aligned(pts2, 8) || !aligned(R_out, 8) || !aligned(t_out, 8) ||
      !aligned(E_out, 8) || !aligned(info_out, 4) || !aligned(found, 4) || !aligned(scratch, 16))
    return handleless_fail(COTR_ERR_ARG, "cotr_refine_pose: doubles must be 8-byte, ints 4-byte and scratch 16-byte aligned");
  const RfPlan l = rp_plan(n);
  if (scratch_bytes < l.bytes) return handleless_fail(COTR_ERR_ARG, "cotr_refine_pose: scratch is smaller than cotr_refine_pose_scratch_bytes");
  char* base = static_cast<char*>(scratch);
  double* xn = reinterpret_cast<double*>(base);
  RpState* st = reinterpret_cast<RpState*>(base + l.state);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(es_normalise_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pts1, pts2, n, k1, k2, xn);
  hipLaunchKernelGGL(rp_init_kernel, dim3(1), dim3(64), 0, s, R_in, t_in, found, st);
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(rp_mask_kernel, dim3((unsigned)l.chunks), dim3(RS_COUNT_THREADS), 0, s, xn, n, mask_in, r == 0, (float)(thr * thr),
                       distance_thresh, r, st, mask_out);
    // pair j judges step j - 1 and takes step j; the round's last one takes none
    for (int j = 0; j <= refine_iters; ++j)
      rf_enqueue_pair<RpTerms>(s, l, scratch, {xn}, n, mask_out, rp_finish_kernel, r, (int)(j == refine_iters),
                               (int)(r == rounds - 1 && j == refine_iters), R_out, t_out, E_out, info_out);
  }
  return launched();
}

}  // extern "C"
