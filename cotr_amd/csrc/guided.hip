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
// cotr_ransac_fundamental: four launches, the last three those of ransac.h's frame on the model FmModel:
//   1. fm_solve_kernel          one thread per iteration: counter-based sample of 7 distinct indices, Hartley normalisation,
//                               null space of the 7x9 system by full-pivot elimination (in LDS), det cubic, up to 3 candidates
//   2. rs_count_kernel<FmModel> grid (3 * max_iters slots) x (2048-point chunks): symmetric epipolar error
//   3. rs_select_kernel<7, 3>   one workgroup replays the sequential selection loop on the counts
//   4. rs_mask_kernel<FmModel>  the chosen candidate's mask (same error code as 2) and F_out
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

// the model of ransac.h's frame: up to 3 candidates per 7-point sample, no tail
struct FmModel {
  static constexpr int MODEL = RS_MODEL, SLOTS = 3;
  using Points = RsPixelPairs;
  struct Tail {};

  // the symmetric epipolar error of DESIGN.md 3h, operation order fixed (compiled without contraction)
  static __device__ __forceinline__ bool inlier(const double* f, const Points& pts, int p, float thr) {
    const double x = f32r(pts.pts1[(size_t)p * 2]), y = f32r(pts.pts1[(size_t)p * 2 + 1]);
    const double u = f32r(pts.pts2[(size_t)p * 2]), v = f32r(pts.pts2[(size_t)p * 2 + 1]);
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

  static __device__ __forceinline__ void tail(const Tail&, int) {}
};

__global__ __launch_bounds__(RS_SOLVE_THREADS) void fm_solve_kernel(const double* __restrict__ pts1, const double* __restrict__ pts2,
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
    RsHartley<RS_MODEL> h;
    bool ok = rs_hartley<RS_MODEL>(pts1, pts2, &shI[lane], RS_SOLVE_THREADS, h);
    const double c1x = h.c1x, c1y = h.c1y, s1 = h.s1, c2x = h.c2x, c2y = h.c2y, s2 = h.s2;
    // 3. rows [x'x, x'y, x', y'x, y'y, y', x, y, 1] in normalised coordinates; full-pivot elimination
    if (ok) {
#pragma unroll
      for (int k = 0; k < RS_MODEL; ++k) {
        const double u1 = (h.x1[k] - c1x) * s1, v1 = (h.y1[k] - c1y) * s1;
        const double u2 = (h.x2[k] - c2x) * s2, v2 = (h.y2[k] - c2y) * s2;
        A_(k, 0) = u2 * u1, A_(k, 1) = u2 * v1, A_(k, 2) = u2;
        A_(k, 3) = v2 * u1, A_(k, 4) = v2 * v1, A_(k, 5) = v2;
        A_(k, 6) = u1, A_(k, 7) = v1, A_(k, 8) = 1.0;
      }
      ok = rs_eliminate<RS_MODEL, 9, 9, RS_SOLVE_THREADS>(&shA[lane], &P_(0));
    }
    if (ok) {
      // 4. the null space: the two free (permuted) columns 7 and 8 set to unit vectors, back substitution
      double f1[9], f2[9];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        double z[9];
        rs_null_vector<RS_MODEL, 9, RS_SOLVE_THREADS>(&shA[lane], RS_MODEL + t, z);
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
        rs_scale9(Fk);
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

// ---- host side ------------------------------------------------------------------------------------------------------
namespace {

struct NnPlan {
  int qblocks[2], splits[2], chunk[2];
  double* pd;   // [splits[0] na + splits[1] nb] the partial minima of both directions
  int* pj;      // and the indices they belong to
  size_t bytes;
};

void nn_split(int nq, int nk, int* qblocks, int* splits, int* chunk) {
  *qblocks = (nq + NN_THREADS - 1) / NN_THREADS;
  const int most = (nk + NN_KALIGN - 1) / NN_KALIGN;
  const int want = min(most, max(1, NN_TARGET_BLOCKS / *qblocks));
  const int per = (nk + want - 1) / want;
  *chunk = (per + NN_KALIGN - 1) / NN_KALIGN * NN_KALIGN;
  *splits = (nk + *chunk - 1) / *chunk;
}

NnPlan nn_plan(void* base, int na, int nb) {
  NnPlan l;
  Carver c(base);
  nn_split(na, nb, &l.qblocks[0], &l.splits[0], &l.chunk[0]);
  nn_split(nb, na, &l.qblocks[1], &l.splits[1], &l.chunk[1]);
  const size_t parts = (size_t)l.splits[0] * na + (size_t)l.splits[1] * nb;
  l.pd = c.take<double>(parts);
  l.pj = c.take<int>(parts);
  l.bytes = c.bytes;
  return l;
}

const char* nn_check_shape(int na, int nb) {
  if (na < 1 || na > NN_MAX_POINTS || nb < 1 || nb > NN_MAX_POINTS) return "na and nb must be in [1, 2^24]";
  return nullptr;
}

const RsEntry FM_ENTRY = {"cotr_ransac_fundamental", "F_out", 15, " (the 7-point LMedS fallback below 15 points is not provided)", FmModel::SLOTS,
                          RS_MAX_ITERS};

}  // namespace

extern "C" {

int cotr_nearest_mutual_scratch_bytes(int na, int nb, size_t* bytes) {
  if (!bytes) return handleless_fail(COTR_ERR_ARG, "cotr_nearest_mutual_scratch_bytes: bytes is NULL");
  if (const char* e = nn_check_shape(na, nb)) return handleless_fail(COTR_ERR_ARG, e);
  *bytes = nn_plan(nullptr, na, nb).bytes;
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
  const NnPlan l = nn_plan(scratch, na, nb);
  if (scratch_bytes < l.bytes) return handleless_fail(COTR_ERR_ARG, "scratch is smaller than cotr_nearest_mutual_scratch_bytes");
  NnArgs a;
  a.dir[0] = NnDir{pred_ab, kp_b, l.pd, l.pj, idx_ab, na, nb, l.qblocks[0], l.splits[0], l.chunk[0]};
  const size_t off = (size_t)l.splits[0] * na;
  a.dir[1] = NnDir{pred_ba, kp_a, l.pd + off, l.pj + off, idx_ba, nb, na, l.qblocks[1], l.splits[1], l.chunk[1]};
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(nn_partial_kernel, dim3(l.qblocks[0] + l.qblocks[1], max(l.splits[0], l.splits[1])), dim3(NN_THREADS), 0, s, a);
  hipLaunchKernelGGL(nn_merge_kernel, dim3((unsigned)(((size_t)na + nb + 255) / 256)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(nn_mutual_kernel, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, s, idx_ab, idx_ba, na, nb, mutual);
  return launched();
}

int cotr_ransac_fundamental_scratch_bytes(int n, int max_iters, size_t* bytes) { return rs_scratch_bytes(FM_ENTRY, n, max_iters, bytes); }

int cotr_ransac_fundamental(const double* pts1, const double* pts2, int n, double threshold, double confidence, int max_iters,
                            uint64_t seed, double* F_out, uint8_t* mask_out, int32_t* info_out, double* hyp_F, int32_t* hyp_count,
                            int32_t* hyp_samples, void* scratch, size_t scratch_bytes, cotr_stream stream) {
  const RsPlan l = rs_plan(FM_ENTRY, max_iters);
  if (const int rc = rs_check_call(FM_ENTRY, n, max_iters, threshold, confidence, pts1, pts2, F_out, mask_out, info_out, hyp_F, hyp_count,
                                   hyp_samples, scratch, scratch_bytes, l.bytes))
    return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const auto solve = [&](double* F, int* count) {
    hipLaunchKernelGGL(fm_solve_kernel, dim3((unsigned)((max_iters + RS_SOLVE_THREADS - 1) / RS_SOLVE_THREADS)), dim3(RS_SOLVE_THREADS), 0, s,
                       pts1, pts2, n, max_iters, seed, F, count, hyp_F, hyp_samples);
  };
  rs_enqueue<FmModel>(s, solve, {pts1, pts2}, n, max_iters, confidence, (float)(threshold * threshold), l, scratch, F_out, mask_out, info_out,
                      hyp_count, {});
  return launched();
}
}  // extern "C"
