// Guided matching of keypoints (demo_guided_matching.py:48-63): nearest keypoint of every predicted position, the mutual
// check, and a fundamental-matrix RANSAC in the structure of OpenCV 3.4's FM_RANSAC.  Rules in DESIGN.md 3h.
//
// cotr_nearest_mutual: three launches on the caller's stream, both directions in each:
//   1. nn_partial_kernel  grid (query blocks of both directions) x (keypoint splits): each workgroup streams its split of
//                         the keypoints through LDS as float64 and keeps, per query, the first minimum of
//                         d = sqrt(dx*dx + dy*dy) (correctly rounded sqrt, no contraction: bit-equal to scipy's
//                         distance_matrix); NaN counts as the minimum, as in numpy's argmin
//   2. nn_merge_kernel    one thread per query: lexicographic minimum of the split partials in split order (lowest j on ties)
//   3. nn_mutual_kernel   mutual[i] = idx_ba[idx_ab[i]] == i
// cotr_ransac_fundamental: four launches:
//   1. rs_solve_kernel    one thread per iteration: counter-based sample of 7 distinct indices, Hartley normalisation,
//                         null space of the 7x9 system by full-pivot elimination (in LDS), det cubic, up to 3 candidates
//   2. rs_count_kernel    grid (3 * max_iters slots) x (2048-point chunks): symmetric epipolar error, ballot + popcount per
//                         wavefront, one integer atomicAdd per wavefront (integer sums: deterministic)
//   3. rs_select_kernel   one workgroup replays the sequential selection loop on the counts (ransac.h, shared with
//                         homography.hip, as are the sampler and the iteration update)
//   4. rs_mask_kernel     the chosen candidate's mask (same error code as 2) and F_out
// No host waits, no allocation: capturable.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "handleless.h"
#include "ransac.h"

using namespace cotr_detail;

#define NN_THREADS 256
#define NN_KALIGN 64           // keypoint splits are multiples of this
#define NN_TARGET_BLOCKS 1024  // query blocks x splits per direction aimed at
#define NN_MAX_POINTS (1 << 24)

#define RS_MODEL 7

// ---- nearest keypoint ---------------------------------------------------------------------------------------------------
struct NnDir {
  const double* q;   // [nq,2] query positions
  const double* k;   // [nk,2] keypoints
  double* pd;        // [splits, nq] partial minima
  int* pj;           // [splits, nq] their indices
  int32_t* idx;      // [nq] result
  int nq, nk, qblocks, splits, chunk;
};
struct NnArgs {
  NnDir dir[2];
};

// first minimum in scan order, NaN smallest (numpy's argmin): bj < 0 means nothing seen yet
__device__ __forceinline__ bool nn_better(double d, double best, int bj) {
  return bj < 0 || d < best || (d != d && best == best);
}

__global__ __launch_bounds__(NN_THREADS) void nn_partial_kernel(NnArgs a) {
  __shared__ double kx[NN_THREADS], ky[NN_THREADS];
  const int dir = (int)blockIdx.x < a.dir[0].qblocks ? 0 : 1;
  const NnDir p = dir == 0 ? a.dir[0] : a.dir[1];
  const int s = blockIdx.y;
  if (s >= p.splits) return;   // uniform over the workgroup
  const int q = ((int)blockIdx.x - (dir == 0 ? 0 : a.dir[0].qblocks)) * NN_THREADS + threadIdx.x;
  const bool active = q < p.nq;
  double px = 0.0, py = 0.0;
  if (active) {
    px = p.q[(size_t)q * 2];
    py = p.q[(size_t)q * 2 + 1];
  }
  const int k0 = s * p.chunk, k1 = min(k0 + p.chunk, p.nk);
  double best = INFINITY;
  int bj = -1;
  for (int t0 = k0; t0 < k1; t0 += NN_THREADS) {
    const int cnt = min(NN_THREADS, k1 - t0);
    __syncthreads();
    if ((int)threadIdx.x < cnt) {
      kx[threadIdx.x] = p.k[(size_t)(t0 + threadIdx.x) * 2];
      ky[threadIdx.x] = p.k[(size_t)(t0 + threadIdx.x) * 2 + 1];
    }
    __syncthreads();
    if (active) {
      for (int t = 0; t < cnt; ++t) {
        const double dx = kx[t] - px, dy = ky[t] - py;
        const double d = sqrt(dx * dx + dy * dy);
        if (nn_better(d, best, bj)) {
          best = d;
          bj = t0 + t;
        }
      }
    }
  }
  if (active) {
    p.pd[(size_t)s * p.nq + q] = best;
    p.pj[(size_t)s * p.nq + q] = bj;
  }
}

__global__ __launch_bounds__(256) void nn_merge_kernel(NnArgs a) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int dir = t < a.dir[0].nq ? 0 : 1;
  const NnDir p = dir == 0 ? a.dir[0] : a.dir[1];
  const int q = t - (dir == 0 ? 0 : a.dir[0].nq);
  if (q >= p.nq) return;
  double best = INFINITY;
  int bj = -1;
  for (int s = 0; s < p.splits; ++s) {   // splits in ascending keypoint order: the first minimum overall
    const double d = p.pd[(size_t)s * p.nq + q];
    const int j = p.pj[(size_t)s * p.nq + q];
    if (nn_better(d, best, bj)) {
      best = d;
      bj = j;
    }
  }
  p.idx[q] = bj;
}

__global__ __launch_bounds__(256) void nn_mutual_kernel(const int32_t* __restrict__ idx_ab, const int32_t* __restrict__ idx_ba,
                                                        int na, int nb, uint8_t* __restrict__ mutual) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= na) return;
  const int j = idx_ab[i];
  mutual[i] = (j >= 0 && j < nb && idx_ba[j] == i) ? 1 : 0;
}

// ---- fundamental-matrix RANSAC ------------------------------------------------------------------------------------------
__device__ __forceinline__ double det3(const double* m) {
  return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// lambda * f1 + (1 - lambda) * f2
__device__ __forceinline__ void pencil(const double* f1, const double* f2, double l, double* f) {
#pragma unroll
  for (int i = 0; i < 9; ++i) f[i] = l * f1[i] + (1.0 - l) * f2[i];
}

// real roots of c3 l^3 + c2 l^2 + c1 l + c0 (Numerical Recipes' trigonometric / Cardano split), ascending
__device__ int cubic_roots(double c3, double c2, double c1, double c0, double* r) {
  int nr = 0;
  if (c3 == 0.0) {
    if (c2 == 0.0) {
      if (c1 != 0.0) r[nr++] = -c0 / c1;
    } else {
      const double disc = c1 * c1 - 4.0 * c2 * c0;
      if (disc == 0.0) {
        r[nr++] = -c1 / (2.0 * c2);
      } else if (disc > 0.0) {
        const double q = -0.5 * (c1 + copysign(sqrt(disc), c1));
        r[nr++] = q / c2;
        r[nr++] = c0 / q;
      }
    }
  } else {
    const double a = c2 / c3, b = c1 / c3, c = c0 / c3;
    const double Q = (a * a - 3.0 * b) / 9.0;
    const double R = (2.0 * a * a * a - 9.0 * a * b + 27.0 * c) / 54.0;
    const double Q3 = Q * Q * Q;
    if (R * R < Q3) {
      const double th = acos(R / sqrt(Q3));
      const double m = -2.0 * sqrt(Q);
      r[0] = m * cos(th / 3.0) - a / 3.0;
      r[1] = m * cos((th + 2.0 * M_PI) / 3.0) - a / 3.0;
      r[2] = m * cos((th - 2.0 * M_PI) / 3.0) - a / 3.0;
      nr = 3;
    } else {
      const double A = -copysign(cbrt(fabs(R) + sqrt(R * R - Q3)), R);
      const double B = A == 0.0 ? 0.0 : Q / A;
      r[0] = (A + B) - a / 3.0;
      nr = 1;
    }
  }
  // ascending (a three-element sorting network; NaN roots stay where they are and make non-finite candidates)
  if (nr >= 2 && r[1] < r[0]) { const double t = r[0]; r[0] = r[1]; r[1] = t; }
  if (nr == 3) {
    if (r[2] < r[1]) { const double t = r[1]; r[1] = r[2]; r[2] = t; }
    if (r[1] < r[0]) { const double t = r[0]; r[0] = r[1]; r[1] = t; }
  }
  return nr;
}

// the symmetric epipolar error of DESIGN.md 3h, operation order fixed (compiled without contraction)
__device__ __forceinline__ bool is_inlier(const double* f, const double* __restrict__ pts1, const double* __restrict__ pts2, int p,
                                          float thr) {
  const double x = f32r(pts1[(size_t)p * 2]), y = f32r(pts1[(size_t)p * 2 + 1]);
  const double u = f32r(pts2[(size_t)p * 2]), v = f32r(pts2[(size_t)p * 2 + 1]);
  const double a = f[0] * x + f[1] * y + f[2];
  const double b = f[3] * x + f[4] * y + f[5];
  const double c = f[6] * x + f[7] * y + f[8];
  const double d2 = u * a + v * b + c;
  const double e2 = d2 * d2 / (a * a + b * b);
  const double at = f[0] * u + f[3] * v + f[6];
  const double bt = f[1] * u + f[4] * v + f[7];
  const double ct = f[2] * u + f[5] * v + f[8];
  const double d1 = x * at + y * bt + ct;
  const double e1 = d1 * d1 / (at * at + bt * bt);
  const float err = (float)(e1 < e2 ? e2 : e1);
  return err <= thr;
}

__global__ __launch_bounds__(RS_SOLVE_THREADS) void rs_solve_kernel(const double* __restrict__ pts1, const double* __restrict__ pts2,
                                                                    int n, int max_iters, uint64_t seed, double* __restrict__ F,
                                                                    int* __restrict__ count, double* __restrict__ hyp_F,
                                                                    int32_t* __restrict__ hyp_samples) {
  // per-thread LDS columns: sh[e * 64 + lane] (the elimination indexes rows and columns at run time)
  __shared__ double shA[63 * RS_SOLVE_THREADS];
  __shared__ double shF[18 * RS_SOLVE_THREADS];
  __shared__ int shI[(RS_MODEL + 9) * RS_SOLVE_THREADS];
  const int lane = threadIdx.x;
  const int it = blockIdx.x * RS_SOLVE_THREADS + lane;
  if (it >= max_iters) return;   // no workgroup barrier below
#define A_(r, c) shA[((r) * 9 + (c)) * RS_SOLVE_THREADS + lane]
#define S_(k) shI[(k) * RS_SOLVE_THREADS + lane]
#define P_(c) shI[(RS_MODEL + (c)) * RS_SOLVE_THREADS + lane]
  // 1. sample: draw d of iteration it is splitmix64(splitmix64(seed) ^ (it << 6 | d)); duplicates are rejected
  const int got = rs_sample<RS_MODEL>(seed, it, n, &shI[lane], RS_SOLVE_THREADS);
  if (hyp_samples) {
    for (int k = 0; k < RS_MODEL; ++k) hyp_samples[(size_t)it * RS_MODEL + k] = k < got ? S_(k) : -1;
  }
  int nr = 0;
  if (got == RS_MODEL) {
    // 2. Hartley normalisation of the 7 pairs (points rounded to float32 first)
    double x1[RS_MODEL], y1[RS_MODEL], x2[RS_MODEL], y2[RS_MODEL];
    double c1x = 0.0, c1y = 0.0, c2x = 0.0, c2y = 0.0;
#pragma unroll
    for (int k = 0; k < RS_MODEL; ++k) {
      const int i = S_(k);
      x1[k] = f32r(pts1[(size_t)i * 2]);
      y1[k] = f32r(pts1[(size_t)i * 2 + 1]);
      x2[k] = f32r(pts2[(size_t)i * 2]);
      y2[k] = f32r(pts2[(size_t)i * 2 + 1]);
      c1x += x1[k], c1y += y1[k], c2x += x2[k], c2y += y2[k];
    }
    c1x /= RS_MODEL, c1y /= RS_MODEL, c2x /= RS_MODEL, c2y /= RS_MODEL;
    double m1 = 0.0, m2 = 0.0;
#pragma unroll
    for (int k = 0; k < RS_MODEL; ++k) {
      const double ax = x1[k] - c1x, ay = y1[k] - c1y, bx = x2[k] - c2x, by = y2[k] - c2y;
      m1 += sqrt(ax * ax + ay * ay);
      m2 += sqrt(bx * bx + by * by);
    }
    m1 /= RS_MODEL, m2 /= RS_MODEL;
    bool ok = m1 > 0.0 && m2 > 0.0 && m1 < INFINITY && m2 < INFINITY;
    const double s1 = M_SQRT2 / m1, s2 = M_SQRT2 / m2;
    // 3. rows [x'x, x'y, x', y'x, y'y, y', x, y, 1] in normalised coordinates; full-pivot elimination
    if (ok) {
#pragma unroll
      for (int k = 0; k < RS_MODEL; ++k) {
        const double u1 = (x1[k] - c1x) * s1, v1 = (y1[k] - c1y) * s1;
        const double u2 = (x2[k] - c2x) * s2, v2 = (y2[k] - c2y) * s2;
        A_(k, 0) = u2 * u1, A_(k, 1) = u2 * v1, A_(k, 2) = u2;
        A_(k, 3) = v2 * u1, A_(k, 4) = v2 * v1, A_(k, 5) = v2;
        A_(k, 6) = u1, A_(k, 7) = v1, A_(k, 8) = 1.0;
      }
      for (int c = 0; c < 9; ++c) P_(c) = c;
      double piv0 = 0.0;
      for (int k = 0; k < RS_MODEL && ok; ++k) {
        double pv = -1.0;
        int pr = k, pc = k;
        for (int r = k; r < RS_MODEL; ++r)
          for (int c = k; c < 9; ++c) {
            const double v = fabs(A_(r, c));
            if (v > pv) pv = v, pr = r, pc = c;
          }
        if (k == 0) piv0 = pv;
        if (!(pv > RS_RANK_TOL * piv0)) {   // also false for NaN
          ok = false;
          break;
        }
        if (pr != k)
          for (int c = 0; c < 9; ++c) {
            const double t = A_(k, c);
            A_(k, c) = A_(pr, c);
            A_(pr, c) = t;
          }
        if (pc != k) {
          for (int r = 0; r < RS_MODEL; ++r) {
            const double t = A_(r, k);
            A_(r, k) = A_(r, pc);
            A_(r, pc) = t;
          }
          const int t = P_(k);
          P_(k) = P_(pc);
          P_(pc) = t;
        }
        const double akk = A_(k, k);
        for (int r = k + 1; r < RS_MODEL; ++r) {
          const double m = A_(r, k) / akk;
          for (int c = k + 1; c < 9; ++c) A_(r, c) = A_(r, c) - m * A_(k, c);
          A_(r, k) = 0.0;
        }
      }
    }
    if (ok) {
      // 4. the null space: the two free (permuted) columns 7 and 8 set to unit vectors, back substitution
      double f1[9], f2[9];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        double z[9];
        z[7] = t == 0 ? 1.0 : 0.0;
        z[8] = t == 0 ? 0.0 : 1.0;
#pragma unroll
        for (int r = RS_MODEL - 1; r >= 0; --r) {
          double acc = 0.0;
#pragma unroll
          for (int c = r + 1; c < 9; ++c) acc += A_(r, c) * z[c];
          z[r] = -acc / A_(r, r);
        }
#pragma unroll
        for (int c = 0; c < 9; ++c) shF[(t * 9 + P_(c)) * RS_SOLVE_THREADS + lane] = z[c];
      }
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        f1[i] = shF[i * RS_SOLVE_THREADS + lane];
        f2[i] = shF[(9 + i) * RS_SOLVE_THREADS + lane];
      }
      // 5. det(l f1 + (1 - l) f2) = c3 l^3 + c2 l^2 + c1 l + c0 from its values at l = 0, 1, -1, 2
      double g[9];
      const double D0 = det3(f2), D1 = det3(f1);
      pencil(f1, f2, -1.0, g);
      const double Dm = det3(g);
      pencil(f1, f2, 2.0, g);
      const double D2 = det3(g);
      const double c0 = D0;
      const double c2 = 0.5 * (D1 + Dm) - D0;
      const double o = 0.5 * (D1 - Dm);
      const double c3 = (D2 - D0 - 4.0 * c2 - 2.0 * o) / 6.0;
      const double c1 = o - c3;
      double roots[3];
      nr = cubic_roots(c3, c2, c1, c0, roots);
      // 6. each root: denormalise F = T2^T Fn T1, unit Frobenius norm, then F[2,2] = 1 unless |F[2,2]| <= DBL_EPSILON
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (k >= nr) break;
        double fn[9], gm[9];
        pencil(f1, f2, roots[k], fn);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          gm[r * 3 + 0] = fn[r * 3 + 0] * s1;
          gm[r * 3 + 1] = fn[r * 3 + 1] * s1;
          gm[r * 3 + 2] = fn[r * 3 + 0] * (-s1 * c1x) + fn[r * 3 + 1] * (-s1 * c1y) + fn[r * 3 + 2];
        }
        double Fk[9];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          Fk[0 * 3 + c] = s2 * gm[0 * 3 + c];
          Fk[1 * 3 + c] = s2 * gm[1 * 3 + c];
          Fk[2 * 3 + c] = (-s2 * c2x) * gm[0 * 3 + c] + (-s2 * c2y) * gm[1 * 3 + c] + gm[2 * 3 + c];
        }
        double ss = 0.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) ss += Fk[i] * Fk[i];
        const double nrm = sqrt(ss);
#pragma unroll
        for (int i = 0; i < 9; ++i) Fk[i] = Fk[i] / nrm;
        if (fabs(Fk[8]) > DBL_EPSILON) {
          const double f22 = Fk[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) Fk[i] = Fk[i] / f22;
          Fk[8] = 1.0;
        } else {
          double big = Fk[0];   // the first entry of largest magnitude
#pragma unroll
          for (int i = 1; i < 9; ++i)
            if (fabs(Fk[i]) > fabs(big)) big = Fk[i];
          if (big < 0.0) {
#pragma unroll
            for (int i = 0; i < 9; ++i) Fk[i] = -Fk[i];
          }
        }
        const size_t slot = (size_t)it * 3 + k;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
          F[slot * 9 + i] = Fk[i];
          if (hyp_F) hyp_F[slot * 9 + i] = Fk[i];
        }
        count[slot] = 0;
      }
    }
  }
#undef A_
#undef S_
#undef P_
  // 7. the slots 3 * it + k without a candidate: NaN, count -1
  for (int k = nr; k < 3; ++k) {
    const size_t slot = (size_t)it * 3 + k;
    for (int i = 0; i < 9; ++i) {
      F[slot * 9 + i] = NAN;
      if (hyp_F) hyp_F[slot * 9 + i] = NAN;
    }
    count[slot] = -1;
  }
}

__global__ __launch_bounds__(RS_COUNT_THREADS) void rs_count_kernel(const double* __restrict__ pts1, const double* __restrict__ pts2, int n,
                                                                    const double* __restrict__ F, int* __restrict__ count, float thr) {
  const int slot = blockIdx.x;
  if (count[slot] < 0) return;   // no candidate in this slot (uniform)
  double f[9];
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    f[i] = F[(size_t)slot * 9 + i];
    finite = finite && isfinite(f[i]);
  }
  if (!finite) return;           // a non-finite candidate counts 0 inliers
  const int base = blockIdx.y * RS_CHUNK;
  int wc = 0;
#pragma unroll
  for (int s = 0; s < RS_COUNT_STEPS; ++s) {
    const int p = base + s * RS_COUNT_THREADS + threadIdx.x;
    const bool in = p < n && is_inlier(f, pts1, pts2, p, thr);
    wc += __popcll(__ballot(in));
  }
  if ((threadIdx.x & 63) == 0 && wc > 0) atomicAdd(&count[slot], wc);
}

__global__ __launch_bounds__(256) void rs_mask_kernel(const double* __restrict__ pts1, const double* __restrict__ pts2, int n,
                                                      const double* __restrict__ F, const int32_t* __restrict__ info, float thr,
                                                      double* __restrict__ F_out, uint8_t* __restrict__ mask) {
  const int found = info[0], slot = info[3];
  const int p = blockIdx.x * 256 + threadIdx.x;
  double f[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) f[i] = found ? F[(size_t)slot * 9 + i] : 0.0;
  if (p < n) mask[p] = (found && is_inlier(f, pts1, pts2, p, thr)) ? 1 : 0;
  if (p < 9) F_out[p] = found ? F[(size_t)slot * 9 + p] : 0.0;
}

// ---- host side ------------------------------------------------------------------------------------------------------
namespace {

struct NnPlan {
  int qblocks[2], splits[2], chunk[2];
  size_t pd, pj, bytes;
};

void nn_split(int nq, int nk, int* qblocks, int* splits, int* chunk) {
  *qblocks = (nq + NN_THREADS - 1) / NN_THREADS;
  const int most = (nk + NN_KALIGN - 1) / NN_KALIGN;
  const int want = min(most, max(1, NN_TARGET_BLOCKS / *qblocks));
  const int per = (nk + want - 1) / want;
  *chunk = (per + NN_KALIGN - 1) / NN_KALIGN * NN_KALIGN;
  *splits = (nk + *chunk - 1) / *chunk;
}

NnPlan nn_plan(int na, int nb) {
  NnPlan l;
  nn_split(na, nb, &l.qblocks[0], &l.splits[0], &l.chunk[0]);
  nn_split(nb, na, &l.qblocks[1], &l.splits[1], &l.chunk[1]);
  const size_t parts = (size_t)l.splits[0] * na + (size_t)l.splits[1] * nb;
  l.pd = 0;
  l.pj = align_up(parts * sizeof(double));
  l.bytes = l.pj + align_up(parts * sizeof(int));
  return l;
}

const char* nn_check_shape(int na, int nb) {
  if (na < 1 || na > NN_MAX_POINTS || nb < 1 || nb > NN_MAX_POINTS) return "na and nb must be in [1, 2^24]";
  return nullptr;
}

struct RsPlan {
  size_t F, count, bytes;
};

RsPlan rs_plan(int max_iters) {
  RsPlan l;
  const size_t slots = (size_t)3 * max_iters;
  l.F = 0;
  l.count = align_up(slots * 9 * sizeof(double));
  l.bytes = l.count + align_up(slots * sizeof(int));
  return l;
}

const char* rs_check_shape(int n, int max_iters) {
  if (n < 15 || n > RS_MAX_POINTS) return "n must be in [15, 2^24] (the 7-point LMedS fallback below 15 points is not provided)";
  if (max_iters < 1 || max_iters > RS_MAX_ITERS) return "max_iters must be in [1, 65536]";
  return nullptr;
}

}  // namespace

extern "C" {

int cotr_nearest_mutual_scratch_bytes(int na, int nb, size_t* bytes) {
  if (!bytes) return handleless_fail(COTR_ERR_ARG, "cotr_nearest_mutual_scratch_bytes: bytes is NULL");
  if (const char* e = nn_check_shape(na, nb)) return handleless_fail(COTR_ERR_ARG, e);
  *bytes = nn_plan(na, nb).bytes;
  return COTR_OK;
}

int cotr_nearest_mutual(const double* pred_ab, const double* kp_b, const double* pred_ba, const double* kp_a, int na, int nb,
                        int32_t* idx_ab, int32_t* idx_ba, uint8_t* mutual, void* scratch, size_t scratch_bytes, cotr_stream stream) {
  if (const char* e = nn_check_shape(na, nb)) return handleless_fail(COTR_ERR_ARG, e);
  if (!pred_ab || !kp_b || !pred_ba || !kp_a || !idx_ab || !idx_ba || !mutual || !scratch)
    return handleless_fail(COTR_ERR_ARG, "cotr_nearest_mutual: a pointer is NULL");
  if (!aligned(pred_ab, 8) || !aligned(kp_b, 8) || !aligned(pred_ba, 8) || !aligned(kp_a, 8) || !aligned(idx_ab, 4) ||
      !aligned(idx_ba, 4) || !aligned(scratch, 16))
    return handleless_fail(COTR_ERR_ARG, "cotr_nearest_mutual: points must be 8-byte, indices 4-byte and scratch 16-byte aligned");
  const NnPlan l = nn_plan(na, nb);
  if (scratch_bytes < l.bytes) return handleless_fail(COTR_ERR_ARG, "scratch is smaller than cotr_nearest_mutual_scratch_bytes");
  char* base = static_cast<char*>(scratch);
  double* pd = reinterpret_cast<double*>(base + l.pd);
  int* pj = reinterpret_cast<int*>(base + l.pj);
  NnArgs a;
  a.dir[0] = NnDir{pred_ab, kp_b, pd, pj, idx_ab, na, nb, l.qblocks[0], l.splits[0], l.chunk[0]};
  const size_t off = (size_t)l.splits[0] * na;
  a.dir[1] = NnDir{pred_ba, kp_a, pd + off, pj + off, idx_ba, nb, na, l.qblocks[1], l.splits[1], l.chunk[1]};
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(nn_partial_kernel, dim3(l.qblocks[0] + l.qblocks[1], max(l.splits[0], l.splits[1])), dim3(NN_THREADS), 0, s, a);
  hipLaunchKernelGGL(nn_merge_kernel, dim3((unsigned)(((size_t)na + nb + 255) / 256)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(nn_mutual_kernel, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, s, idx_ab, idx_ba, na, nb, mutual);
  return launched();
}

int cotr_ransac_fundamental_scratch_bytes(int n, int max_iters, size_t* bytes) {
  if (!bytes) return handleless_fail(COTR_ERR_ARG, "cotr_ransac_fundamental_scratch_bytes: bytes is NULL");
  if (const char* e = rs_check_shape(n, max_iters)) return handleless_fail(COTR_ERR_ARG, e);
  *bytes = rs_plan(max_iters).bytes;
  return COTR_OK;
}

int cotr_ransac_fundamental(const double* pts1, const double* pts2, int n, double threshold, double confidence, int max_iters,
                            uint64_t seed, double* F_out, uint8_t* mask_out, int32_t* info_out, double* hyp_F, int32_t* hyp_count,
                            int32_t* hyp_samples, void* scratch, size_t scratch_bytes, cotr_stream stream) {
  if (const char* e = rs_check_shape(n, max_iters)) return handleless_fail(COTR_ERR_ARG, e);
  if (!(threshold > 0.0) || !(threshold < INFINITY)) return handleless_fail(COTR_ERR_ARG, "threshold must be finite and > 0");
  if (!(confidence > 0.0 && confidence < 1.0)) return handleless_fail(COTR_ERR_ARG, "confidence must be in (0, 1)");
  if (!pts1 || !pts2 || !F_out || !mask_out || !info_out || !scratch)
    return handleless_fail(COTR_ERR_ARG, "cotr_ransac_fundamental: pts1, pts2, F_out, mask_out, info_out and scratch must not be NULL");
  if (!aligned(pts1, 8) || !aligned(pts2, 8) || !aligned(F_out, 8) || !aligned(info_out, 4) || !aligned(hyp_F, 8) ||
      !aligned(hyp_count, 4) || !aligned(hyp_samples, 4) || !aligned(scratch, 16))
    return handleless_fail(COTR_ERR_ARG, "cotr_ransac_fundamental: doubles must be 8-byte, ints 4-byte and scratch 16-byte aligned");
  const RsPlan l = rs_plan(max_iters);
  if (scratch_bytes < l.bytes) return handleless_fail(COTR_ERR_ARG, "scratch is smaller than cotr_ransac_fundamental_scratch_bytes");
  char* base = static_cast<char*>(scratch);
  double* F = reinterpret_cast<double*>(base + l.F);
  int* count = reinterpret_cast<int*>(base + l.count);
  const float thr = (float)(threshold * threshold);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(rs_solve_kernel, dim3((unsigned)((max_iters + RS_SOLVE_THREADS - 1) / RS_SOLVE_THREADS)), dim3(RS_SOLVE_THREADS), 0, s,
                     pts1, pts2, n, max_iters, seed, F, count, hyp_F, hyp_samples);
  hipLaunchKernelGGL(rs_count_kernel, dim3((unsigned)(3 * max_iters), (unsigned)((n + RS_CHUNK - 1) / RS_CHUNK)), dim3(RS_COUNT_THREADS), 0,
                     s, pts1, pts2, n, F, count, thr);
  hipLaunchKernelGGL((rs_select_kernel<RS_MODEL, 3>), dim3(1), dim3(RS_SELECT_THREADS), 0, s, count, max_iters, n, confidence, info_out, hyp_count);
  hipLaunchKernelGGL(rs_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pts1, pts2, n, F, info_out, thr, F_out, mask_out);
  return launched();
}

}  // extern "C"
