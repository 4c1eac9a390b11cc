// Rigid and similarity registration of 3D-3D correspondences: 3-point RANSAC on Horn's closed form with a closed-form refit
// on the inliers (absolute orientation: Kabsch / Horn / Umeyama).  Rules in DESIGN.md 3h-8.  y = s R x + t.
//
// cotr_ransac_rigid3d: 4 launches with rounds = 0, else 4 + 4 + 6 (rounds - 1) on the caller's stream:
//   1. rg_solve_kernel          one thread per iteration: counter-based sample of 3 distinct indices, the centred 3 x 3
//                               cross-covariance of the three pairs, Horn's 4 x 4 matrix, its largest eigenvector by cyclic
//                               Jacobi, Umeyama's scale
//   2. rs_count_kernel<RgModel> grid (max_iters slots) x (2048-point chunks): squared distance of s R x + t from y
//   3. rs_select_kernel<3, 1>   the sequential selection loop replayed on the counts
//   4. rs_mask_kernel<RgModel>  the chosen candidate's mask; (the model's tail) R_out, t_out, scale_out, info[4..7], the
//      refit's state      (2 - 4: ransac.h's frame on the model RgModel, as is the sampler of 1)
//   5. per round: (from round 2 on) rg_mask_kernel, the inliers of the current model among all n points -> the round's mask
//      in scratch and its count; rf_accum_kernel<RgSums1> / rg_centroid_kernel (the count and the six coordinate sums -> the
//      two centroids); rf_accum_kernel<RgSums2> / rg_fit_kernel (the nine centred cross-covariance sums, sum |a'|^2, the
//      squared error of the current model -> Horn's closed form again, the outputs); (from round 2 on) rg_commit_kernel: the
//      round's mask -> mask_out if the round was executed.  refit.h's frame with two terms policies.
//      A device-side flag idles the chain from the first round that is skipped; its length never depends on the data.
// A candidate is 9 doubles: rows 1 and 2 of s R, then t; row 3 is rebuilt by rg_expand wherever the candidate is used.
// No floating-point atomics: the same input gives the same bits.  No host waits, no allocation: capturable.
// Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "handleless.h"
#include "ransac.h"
#include "refit.h"

using namespace cotr_detail;

#define RG_MODEL 3
#define RG_SUMS1 7             // the count, the sums of x, the sums of y
#define RG_SUMS2 11            // the 9 centred cross-covariance sums, sum |a'|^2, the squared error of the current model
#define RG_STRIDE 11           // the row length of the per-chunk sums, shared by both passes
#define RG_MAX_ROUNDS 8

// ---- a candidate ------------------------------------------------------------------------------------------------------
// m[9] = rows 1 and 2 of s R, t -> all of s R and s: s = |row 1| and row 3 = (row 1 x row 2) / s with a scale, s = 1
// exactly and row 3 = row 1 x row 2 without
RS_HD __forceinline__ void rg_expand(const double* m, int with_scale, double* sR, double* s) {
  const double c0 = m[1] * m[5] - m[2] * m[4], c1 = m[2] * m[3] - m[0] * m[5], c2 = m[0] * m[4] - m[1] * m[3];
  const double n = with_scale ? sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]) : 1.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) sR[i] = m[i];
  sR[6] = with_scale ? c0 / n : c0, sR[7] = with_scale ? c1 / n : c1, sR[8] = with_scale ? c2 / n : c2;
  *s = n;
}

// |s R x + t - y|^2 with all of s R given, summed left to right
RS_HD __forceinline__ double rg_error(const double* sR, const double* t, const double* x, const double* y) {
  const double dx = (((sR[0] * x[0] + sR[1] * x[1]) + sR[2] * x[2]) + t[0]) - y[0];
  const double dy = (((sR[3] * x[0] + sR[4] * x[1]) + sR[5] * x[2]) + t[1]) - y[1];
  const double dz = (((sR[6] * x[0] + sR[7] * x[1]) + sR[8] * x[2]) + t[2]) - y[2];
  return (dx * dx + dy * dy) + dz * dz;
}

// float(squared distance) <= thr; false for NaN
__device__ __forceinline__ bool rg_inlier(const double* sR, const double* t, const double* __restrict__ src,
                                          const double* __restrict__ dst, int p, float thr) {
  const double x[3] = {src[(size_t)p * 3], src[(size_t)p * 3 + 1], src[(size_t)p * 3 + 2]};
  const double y[3] = {dst[(size_t)p * 3], dst[(size_t)p * 3 + 1], dst[(size_t)p * 3 + 2]};
  return (float)rg_error(sR, t, x, y) <= thr;
}

// Horn's closed form on moments: S[j * 3 + i] = sum a'_j b'_i (a' = x - ca, b' = y - cb), saa = sum |a'|^2.  The symmetric
// 4 x 4 matrix N of the quaternion method, its eigenvectors by rs_jacobi<4>; q = the eigenvector of the first largest
// eigenvalue l1, made a unit vector; R from q (a proper rotation by construction); s = sum_ij R_ij S_ji / saa with a scale
// (finite and > 0), else 1; t = cb - s R ca.  false when the moments are degenerate: l1 is not finite and > 0, or is not
// separated from the second largest eigenvalue l2, l1 - l2 <= RS_RANK_TOL l1 (collinear points), or the scale fails.
__device__ __forceinline__ bool rg_horn(const double* S, double saa, const double* ca, const double* cb, int with_scale, double* sR, double* t,
                                        double* s_out) {
  const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
  double a[4][4], v[4][4];
  a[0][0] = (Sxx + Syy) + Szz, a[0][1] = Syz - Szy, a[0][2] = Szx - Sxz, a[0][3] = Sxy - Syx;
  a[1][1] = (Sxx - Syy) - Szz, a[1][2] = Sxy + Syx, a[1][3] = Szx + Sxz;
  a[2][2] = (Syy - Sxx) - Szz, a[2][3] = Syz + Szy;
  a[3][3] = (Szz - Sxx) - Syy;
  a[1][0] = a[0][1], a[2][0] = a[0][2], a[3][0] = a[0][3], a[2][1] = a[1][2], a[3][1] = a[1][3], a[3][2] = a[2][3];
  rs_jacobi<4>(a, v);
  // the first largest eigenvalue and the largest of the others, without indexing registers at run time
  double l1 = a[0][0];
  int k = 0;
  if (a[1][1] > l1) l1 = a[1][1], k = 1;
  if (a[2][2] > l1) l1 = a[2][2], k = 2;
  if (a[3][3] > l1) l1 = a[3][3], k = 3;
  double l2 = -INFINITY;
  if (k != 0 && a[0][0] > l2) l2 = a[0][0];
  if (k != 1 && a[1][1] > l2) l2 = a[1][1];
  if (k != 2 && a[2][2] > l2) l2 = a[2][2];
  if (k != 3 && a[3][3] > l2) l2 = a[3][3];
  if (!(l1 > 0.0) || !(l1 < INFINITY) || !(l1 - l2 > RS_RANK_TOL * l1)) return false;   // also for NaN
  double q[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = k == 0 ? v[i][0] : (k == 1 ? v[i][1] : (k == 2 ? v[i][2] : v[i][3]));
  const double qn = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  const double w = q[0] / qn, x = q[1] / qn, y = q[2] / qn, z = q[3] / qn;
  double R[9];
  R[0] = ((w * w + x * x) - y * y) - z * z, R[1] = 2.0 * (x * y - w * z), R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z), R[4] = ((w * w - x * x) + y * y) - z * z, R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y), R[7] = 2.0 * (y * z + w * x), R[8] = ((w * w - x * x) - y * y) + z * z;
  double s = 1.0;
  if (with_scale) {
    double num = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) num += R[i * 3 + j] * S[j * 3 + i];
    s = num / saa;
    if (!(s > 0.0) || !(s < INFINITY)) return false;
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = s * R[i];
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) sR[i] = R[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = cb[i] - ((R[i * 3] * ca[0] + R[i * 3 + 1] * ca[1]) + R[i * 3 + 2] * ca[2]);
  *s_out = s;
  return true;
}

// the refit's state, in scratch
struct RgState {
  double sR[9], t[3], s;       // current model
  double err;                  // the squared error of the model before the last fit, on that fit's mask
  double ca[3], cb[3];         // the centroids of the round's mask
  int done;                    // nothing more to accumulate: nothing was found, or a round was skipped
  int with_scale;
  int found;
  int commit;                  // the round was executed: its mask becomes mask_out
  int rounds_run, in_mask;     // info[4], info[5]
  int count[RG_MAX_ROUNDS];    // points in each round's mask: the RANSAC's best count, then the re-counts
};

// the model of ransac.h's frame: one candidate per 3-point sample; the tail writes the chosen model and starts the refit
struct RgModel {
  static constexpr int MODEL = RG_MODEL, SLOTS = 1;
  struct Points {
    const double* __restrict__ src;
    const double* __restrict__ dst;
    int with_scale;
  };
  struct Tail {
    const double* cand;
    int32_t* info;
    double* R_out;
    double* t_out;
    double* scale_out;
    RgState* st;
    int with_scale;
  };

  static __device__ __forceinline__ bool inlier(const double* m, const Points& pts, int p, float thr) {
    double sR[9], s;
    rg_expand(m, pts.with_scale, sR, &s);
    return rg_inlier(sR, m + 6, pts.src, pts.dst, p, thr);
  }

  static __device__ __forceinline__ void tail(const Tail& t, int found) {
    double m[9];
    for (int i = 0; i < 9; ++i) m[i] = found ? t.cand[(size_t)t.info[3] * 9 + i] : 0.0;
    double sR[9], s;
    rg_expand(m, t.with_scale, sR, &s);
    if (!found) s = 0.0;
    for (int i = 0; i < 9; ++i) {
      t.st->sR[i] = sR[i];
      t.R_out[i] = found ? sR[i] / s : 0.0;
    }
    for (int i = 0; i < 3; ++i) t.t_out[i] = t.st->t[i] = m[6 + i];
    t.scale_out[0] = t.st->s = s;
    t.st->err = 0.0;
    t.st->done = found ? 0 : 1;
    t.st->with_scale = t.with_scale;
    t.st->found = found;
    t.st->commit = 0;
    t.st->rounds_run = 0;
    t.st->in_mask = found ? t.info[1] : 0;
    for (int i = 0; i < 3; ++i) t.st->ca[i] = t.st->cb[i] = 0.0;
    for (int r = 0; r < RG_MAX_ROUNDS; ++r) t.st->count[r] = 0;
    t.st->count[0] = t.st->in_mask;
    t.info[4] = 0;
    t.info[5] = t.st->in_mask;
    t.info[6] = 0;
    t.info[7] = 0;
  }
};

// ---- the solve --------------------------------------------------------------------------------------------------------
// whether the three points p[k * 3 + i] lie on a line: |e1 x e2| <= RS_RANK_TOL |e1| |e2| (true for NaN too)
__device__ __forceinline__ bool rg_collinear(const double* p) {
  const double e1x = p[3] - p[0], e1y = p[4] - p[1], e1z = p[5] - p[2];
  const double e2x = p[6] - p[0], e2y = p[7] - p[1], e2z = p[8] - p[2];
  const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  const double nn = sqrt(nx * nx + ny * ny + nz * nz);
  const double l1 = sqrt(e1x * e1x + e1y * e1y + e1z * e1z), l2 = sqrt(e2x * e2x + e2y * e2y + e2z * e2z);
  return !(nn > RS_RANK_TOL * (l1 * l2));
}

__global__ __launch_bounds__(RS_SOLVE_THREADS) void rg_solve_kernel(const double* __restrict__ src, const double* __restrict__ dst, int n,
                                                                    int max_iters, uint64_t seed, int with_scale, double* __restrict__ cand,
                                                                    int* __restrict__ count, double* __restrict__ hyp_model,
                                                                    int32_t* __restrict__ hyp_samples) {
  __shared__ int shI[RG_MODEL * RS_SOLVE_THREADS];   // the sample: the sampler indexes it at run time
  const int lane = threadIdx.x;
  const int it = blockIdx.x * RS_SOLVE_THREADS + lane;
  if (it >= max_iters) return;   // no workgroup barrier below
#define S_(k) shI[(k) * RS_SOLVE_THREADS + lane]
  const int got = rs_sample<RG_MODEL>(seed, it, n, &shI[lane], RS_SOLVE_THREADS);
  if (hyp_samples) {
    for (int j = 0; j < RG_MODEL; ++j) hyp_samples[(size_t)it * RG_MODEL + j] = j < got ? S_(j) : -1;
  }
  bool ok = got == RG_MODEL;
  double m[9];
  if (ok) {
    double a[9], b[9];
    bool finite = true;
#pragma unroll
    for (int j = 0; j < RG_MODEL; ++j) {
      const int i = S_(j);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        a[j * 3 + c] = src[(size_t)i * 3 + c];
        b[j * 3 + c] = dst[(size_t)i * 3 + c];
        finite = finite && a[j * 3 + c] == a[j * 3 + c] && b[j * 3 + c] == b[j * 3 + c];
      }
    }
    ok = finite && !rg_collinear(a) && !rg_collinear(b);
    if (ok) {
      double ca[3], cb[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        ca[c] = ((a[c] + a[3 + c]) + a[6 + c]) / 3.0;
        cb[c] = ((b[c] + b[3 + c]) + b[6 + c]) / 3.0;
      }
      double S[9], saa = 0.0;
#pragma unroll
      for (int i = 0; i < 9; ++i) S[i] = 0.0;
#pragma unroll
      for (int j = 0; j < RG_MODEL; ++j) {
        const double ax = a[j * 3] - ca[0], ay = a[j * 3 + 1] - ca[1], az = a[j * 3 + 2] - ca[2];
        const double bx = b[j * 3] - cb[0], by = b[j * 3 + 1] - cb[1], bz = b[j * 3 + 2] - cb[2];
        S[0] += ax * bx, S[1] += ax * by, S[2] += ax * bz;
        S[3] += ay * bx, S[4] += ay * by, S[5] += ay * bz;
        S[6] += az * bx, S[7] += az * by, S[8] += az * bz;
        saa += (ax * ax + ay * ay) + az * az;
      }
      double sR[9], t[3], s;
      ok = rg_horn(S, saa, ca, cb, with_scale, sR, t, &s);
#pragma unroll
      for (int i = 0; i < 6; ++i) m[i] = sR[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) m[6 + i] = t[i];
    }
  }
#undef S_
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const double v = ok ? m[i] : NAN;   // a slot without a candidate: NaN, count -1
    cand[(size_t)it * 9 + i] = v;
    if (hyp_model) hyp_model[(size_t)it * 9 + i] = v;
  }
  count[it] = ok ? 0 : -1;
}

// ---- the refit ------------------------------------------------------------------------------------------------------------
// pass 1: the count and the coordinate sums of the masked pairs
struct RgSums1 {
  static constexpr int SUMS = RG_SUMS1, STRIDE = RG_STRIDE;
  using Points = RgModel::Points;
  using State = RgState;
  static __device__ __forceinline__ void terms(const RgState* __restrict__, const Points& pts, int p, double* acc) {
    acc[0] += 1.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      acc[1 + c] += pts.src[(size_t)p * 3 + c];
      acc[4 + c] += pts.dst[(size_t)p * 3 + c];
    }
  }
};

// pass 2: about the centroids of pass 1, and the squared error of the current model
struct RgSums2 {
  static constexpr int SUMS = RG_SUMS2, STRIDE = RG_STRIDE;
  using Points = RgModel::Points;
  using State = RgState;
  static __device__ __forceinline__ void terms(const RgState* __restrict__ st, const Points& pts, int p, double* acc) {
    const double x[3] = {pts.src[(size_t)p * 3], pts.src[(size_t)p * 3 + 1], pts.src[(size_t)p * 3 + 2]};
    const double y[3] = {pts.dst[(size_t)p * 3], pts.dst[(size_t)p * 3 + 1], pts.dst[(size_t)p * 3 + 2]};
    const double ax = x[0] - st->ca[0], ay = x[1] - st->ca[1], az = x[2] - st->ca[2];
    const double bx = y[0] - st->cb[0], by = y[1] - st->cb[1], bz = y[2] - st->cb[2];
    acc[0] += ax * bx, acc[1] += ax * by, acc[2] += ax * bz;
    acc[3] += ay * bx, acc[4] += ay * by, acc[5] += ay * bz;
    acc[6] += az * bx, acc[7] += az * by, acc[8] += az * bz;
    acc[9] += (ax * ax + ay * ay) + az * az;
    acc[10] += rg_error(st->sR, st->t, x, y);
  }
};

// The mask of a later round and its count: the inliers of the current model among all n points -> work[n].  Idle once the
// chain is.
__global__ __launch_bounds__(RS_COUNT_THREADS) void rg_mask_kernel(RgModel::Points pts, int n, float thr, int round, RgState* __restrict__ st,
                                                                   uint8_t* __restrict__ work) {
  if (st->done) return;   // uniform
  double sR[9], t[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) sR[i] = st->sR[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = st->t[i];
  const int base = blockIdx.x * RS_CHUNK;
  int wc = 0;
#pragma unroll 1
  for (int s = 0; s < RS_COUNT_STEPS; ++s) {
    const int p = base + s * RS_COUNT_THREADS + threadIdx.x;
    const bool in = p < n && rg_inlier(sR, t, pts.src, pts.dst, p, thr);
    if (p < n) work[p] = in ? 1 : 0;
    wc += __popcll(__ballot(in));
  }
  if ((threadIdx.x & 63) == 0 && wc > 0) atomicAdd(&st->count[round], wc);
}

// after pass 1: the centroids of the round's mask; fewer than 3 points in it: the round is skipped and the chain idles
__global__ __launch_bounds__(64) void rg_centroid_kernel(int chunks, const double* __restrict__ parts, RgState* __restrict__ st, int round) {
  __shared__ double sums[RG_STRIDE];
  const bool active = !st->done;   // uniform; read before anything below writes it
  rf_reduce<RG_STRIDE>(parts, chunks, active ? RG_SUMS1 : 0, sums);
  if (threadIdx.x != 0) return;
  st->commit = 0;
  if (!active) return;
  if (st->count[round] < RG_MODEL) {
    st->done = 1;
    return;
  }
  const double cnt = sums[0];
  for (int c = 0; c < 3; ++c) {
    st->ca[c] = sums[1 + c] / cnt;
    st->cb[c] = sums[4 + c] / cnt;
  }
}

// after pass 2: Horn's closed form on the round's moments; degenerate moments: the round is skipped, the model stays and
// the chain idles.  Writes the outputs from the state.
__global__ __launch_bounds__(64) void rg_fit_kernel(int chunks, const double* __restrict__ parts, RgState* __restrict__ st, int round,
                                                    double* __restrict__ R_out, double* __restrict__ t_out, double* __restrict__ scale_out,
                                                    int32_t* __restrict__ info) {
  __shared__ double sums[RG_STRIDE];
  const bool active = !st->done;   // uniform; read before anything below writes it
  rf_reduce<RG_STRIDE>(parts, chunks, active ? RG_SUMS2 : 0, sums);
  if (threadIdx.x != 0) return;
  if (active) {
    double S[9], ca[3], cb[3], sR[9], t[3], s;
    for (int i = 0; i < 9; ++i) S[i] = sums[i];
    for (int i = 0; i < 3; ++i) ca[i] = st->ca[i], cb[i] = st->cb[i];
    if (rg_horn(S, sums[9], ca, cb, st->with_scale, sR, t, &s)) {
      for (int i = 0; i < 9; ++i) st->sR[i] = sR[i];
      for (int i = 0; i < 3; ++i) st->t[i] = t[i];
      st->s = s;
      st->err = sums[10];
      st->rounds_run = st->rounds_run + 1;
      st->in_mask = st->count[round];
      st->commit = 1;
    } else {
      st->done = 1;
    }
  }
  const int found = st->found;
  const double s = st->s;
  for (int i = 0; i < 9; ++i) R_out[i] = found ? st->sR[i] / s : 0.0;
  for (int i = 0; i < 3; ++i) t_out[i] = found ? st->t[i] : 0.0;
  scale_out[0] = found ? s : 0.0;
  info[4] = st->rounds_run;
  info[5] = st->in_mask;
}

// the mask of a later round that was executed -> mask_out
__global__ __launch_bounds__(256) void rg_commit_kernel(int n, const RgState* __restrict__ st, const uint8_t* __restrict__ work,
                                                        uint8_t* __restrict__ mask_out) {
  if (!st->commit) return;   // uniform
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p < n) mask_out[p] = work[p];
}

// ---- host side ------------------------------------------------------------------------------------------------------------
namespace {

const RsEntry RG_ENTRY = {"cotr_ransac_rigid3d", "R_out", RG_MODEL, "", RgModel::SLOTS, RS_MAX_ITERS};

// after the frame's candidates and counts: the refit's state, its partial sums [chunks, RG_STRIDE], then the mask of a later
// round [n]
struct RgPlan {
  RfPlan rf;
  uint8_t* work;
  size_t bytes;
};

RgPlan rg_plan(void* base, const RsPlan& rs, int n) {
  RgPlan l;
  l.rf = rf_plan(rs.bytes, sizeof(RgState), n, RG_STRIDE);
  Carver c(base, l.rf.bytes);
  l.work = c.take<uint8_t>(n);
  l.bytes = c.bytes;
  return l;
}

}  // namespace

extern "C" {

int cotr_ransac_rigid3d_scratch_bytes(int n, int max_iters, size_t* bytes) {
  if (const int rc = rs_scratch_bytes(RG_ENTRY, n, max_iters, bytes)) return rc;
  *bytes = rg_plan(nullptr, rs_plan(RG_ENTRY, max_iters), n).bytes;
  return COTR_OK;
}

int cotr_ransac_rigid3d(const double* src, const double* dst, int n, double threshold, double confidence, int max_iters, uint64_t seed,
                        int with_scale, int rounds, double* R_out, double* t_out, double* scale_out, uint8_t* mask_out, int32_t* info_out,
                        double* hyp_model, int32_t* hyp_count, int32_t* hyp_samples, void* scratch, size_t scratch_bytes, cotr_stream stream) {
  const RsPlan rs = rs_plan(RG_ENTRY, max_iters);
  const RgPlan l = rg_plan(scratch, rs, n);
  if (const int rc = rs_check_call(RG_ENTRY, n, max_iters, threshold, confidence, src, dst, R_out, mask_out, info_out, hyp_model, hyp_count,
                                   hyp_samples, scratch, scratch_bytes, l.bytes))
    return rc;
  if (!t_out || !scale_out) return rs_fail(RG_ENTRY, "t_out and scale_out must not be NULL");
  if (!aligned(t_out, 8) || !aligned(scale_out, 8)) return rs_fail(RG_ENTRY, "t_out and scale_out must be 8-byte aligned");
  if (with_scale != 0 && with_scale != 1) return rs_fail(RG_ENTRY, "with_scale must be 0 or 1");
  if (rounds < 0 || rounds > RG_MAX_ROUNDS) return rs_fail(RG_ENTRY, "rounds must be in [0, 8]");
  const float thr = (float)(threshold * threshold);
  if (!(thr > 0.0f) || !(thr < INFINITY)) return rs_fail(RG_ENTRY, "the squared threshold must be a finite float32 that is not 0");
  char* base = static_cast<char*>(scratch);
  const double* cand = reinterpret_cast<const double*>(base + rs.candidates);
  RgState* st = reinterpret_cast<RgState*>(base + l.rf.state);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const auto solve = [&](double* c, int* count) {
    hipLaunchKernelGGL(rg_solve_kernel, dim3((unsigned)((max_iters + RS_SOLVE_THREADS - 1) / RS_SOLVE_THREADS)), dim3(RS_SOLVE_THREADS), 0, s, src,
                       dst, n, max_iters, seed, with_scale, c, count, hyp_model, hyp_samples);
  };
  const RgModel::Points pts = {src, dst, with_scale};
  rs_enqueue<RgModel>(s, solve, pts, n, max_iters, confidence, thr, rs, scratch, nullptr, mask_out, info_out, hyp_count,
                      {cand, info_out, R_out, t_out, scale_out, st, with_scale});
  for (int r = 0; r < rounds; ++r) {
    // round 1 fits on the RANSAC mask, a later one on its own re-count
    const uint8_t* mask = r == 0 ? mask_out : l.work;
    if (r > 0)
      hipLaunchKernelGGL(rg_mask_kernel, dim3((unsigned)l.rf.chunks), dim3(RS_COUNT_THREADS), 0, s, pts, n, thr, r, st, l.work);
    rf_enqueue_pair<RgSums1>(s, l.rf, scratch, pts, n, mask, rg_centroid_kernel, r);
    rf_enqueue_pair<RgSums2>(s, l.rf, scratch, pts, n, mask, rg_fit_kernel, r, R_out, t_out, scale_out, info_out);
    if (r > 0) hipLaunchKernelGGL(rg_commit_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, (const RgState*)st, (const uint8_t*)l.work, mask_out);
  }
  return launched();
}

}  // extern "C"
