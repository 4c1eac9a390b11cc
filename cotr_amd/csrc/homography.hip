// Homography RANSAC with a least-squares refit on the inliers, in the structure of OpenCV's findHomography(RANSAC).
// Rules in DESIGN.md 3h-2.  H maps pts1 to pts2: [u, v, 1]^T ~ H [x, y, 1]^T.
//
// cotr_ransac_homography: 4 + 2 * (3 + refine_iters + 1) launches on the caller's stream (4 + 2 * 3 with refine_iters = 0):
//   1. hg_solve_kernel          one thread per iteration: counter-based sample of 4 distinct indices, cv2's checkSubset, Hartley
//                               normalisation, the 8x8 system of get_perspective_transform by full-pivot elimination (LDS)
//   2. rs_count_kernel<HgModel> grid (max_iters slots) x (2048-point chunks): transfer error
//   3. rs_select_kernel<4, 1>   the sequential selection loop replayed on the counts
//   4. rs_mask_kernel<HgModel>  the chosen candidate's mask, H_ransac, and (the model's tail) the refit's state
//      (2 - 4: ransac.h's frame on the model HgModel, as are the sampler, the normalisation and the elimination of 1)
//   5. the refit chain, pairs of rf_accum_kernel<HgTerms<STAGE>> (per 2048-point chunk: up to 45 sums over the mask, every
//      thread over its points in order, every wavefront in a fixed tree, the 4 wavefronts in order -> scratch) and
//      hg_finish_kernel (one workgroup: the chunks in chunk order, then the stage's small serial problem); refit.h's frame:
//        CENTROID, DISTANCE          the Hartley normalisation of the inliers
//        DLT                         L^T L (45 sums) -> the eigenvector of the smallest eigenvalue by cyclic Jacobi
//        GN x (refine_iters + 1)     (none with refine_iters = 0) J^T J, J^T r, squared error (45 sums) -> rf_step: accept or undo the last step, take the next
//      A device-side flag ends the chain's work early; its length never depends on the data.
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

#define HG_MODEL 4
#define HG_SUMS 45
#define HG_MAX_REFINE 64
#define HG_H22_TOL 1e-12       // |Hn[2,2]| <= this times ||Hn||: the DLT result is kept as it is

enum { HG_CENTROID = 0, HG_DISTANCE = 1, HG_DLT = 2, HG_GN = 3 };

// the refit's state, in scratch; written by the mask kernel's tail (done, status, kept, trial) and by the finish kernels
// and the model of refit.h's step: the 8 free entries of Hn
struct HgState : RfCore {
  double c1x, c1y, s1, c2x, c2y, s2;   // T = [[s, 0, -s cx], [0, s, -s cy], [0, 0, 1]] of each point set
  double cnt;                          // number of inliers, as a sum over the mask
  double h[9];                         // current Hn (normalised frame); h[8] = 1 while refining
  double hprev[9];                     // Hn before the step on trial
  int status;                          // 0 DLT + refine, 1 DLT only, 2 none

  static constexpr int PARAMS = 8;
  static __device__ __forceinline__ void judged(HgState* st) { st->status = 0; }
  static __device__ __forceinline__ void save(HgState* st) {
    for (int i = 0; i < 9; ++i) st->hprev[i] = st->h[i];
  }
  static __device__ __forceinline__ void restore(HgState* st) {
    for (int i = 0; i < 9; ++i) st->h[i] = st->hprev[i];
  }
  static __device__ __forceinline__ void apply(HgState* st, const double* d) {
    for (int i = 0; i < 8; ++i) st->h[i] = st->h[i] + d[i];
  }
};

// ---- the model of ransac.h's frame: one candidate per 4-point sample; the tail starts the refit's state -------------------
struct HgModel {
  static constexpr int MODEL = HG_MODEL, SLOTS = 1;
  using Points = RsPixelPairs;
  struct Tail {
    HgState* st;
  };

  static __device__ __forceinline__ float error(const double* h, double x, double y, double u, double v) {
    const double w = 1.0 / (h[6] * x + h[7] * y + h[8]);
    const double dx = (h[0] * x + h[1] * y + h[2]) * w - u;
    const double dy = (h[3] * x + h[4] * y + h[5]) * w - v;
    return (float)(dx * dx + dy * dy);
  }

  static __device__ __forceinline__ bool inlier(const double* h, const Points& pts, int p, float thr) {
    const double x = f32r(pts.pts1[(size_t)p * 2]), y = f32r(pts.pts1[(size_t)p * 2 + 1]);
    const double u = f32r(pts.pts2[(size_t)p * 2]), v = f32r(pts.pts2[(size_t)p * 2 + 1]);
    return error(h, x, y, u, v) <= thr;   // false for NaN
  }

  static __device__ __forceinline__ void tail(const Tail& t, int found) {
    t.st->done = found ? 0 : 1;
    t.st->status = 2;
    t.st->kept = 0;
    t.st->trial = 0;
  }
};

// H = T2^-1 Hn T1
__device__ __forceinline__ void hg_denormalise(const double* hn, double c1x, double c1y, double s1, double c2x, double c2y, double s2,
                                               double* H) {
  double gm[9];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    gm[r * 3 + 0] = hn[r * 3 + 0] * s1;
    gm[r * 3 + 1] = hn[r * 3 + 1] * s1;
    gm[r * 3 + 2] = hn[r * 3 + 0] * (-s1 * c1x) + hn[r * 3 + 1] * (-s1 * c1y) + hn[r * 3 + 2];
  }
  const double i2 = 1.0 / s2;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    H[0 * 3 + c] = i2 * gm[0 * 3 + c] + c2x * gm[2 * 3 + c];
    H[1 * 3 + c] = i2 * gm[1 * 3 + c] + c2y * gm[2 * 3 + c];
    H[2 * 3 + c] = gm[2 * 3 + c];
  }
}

// cv2's checkSubset on the 4 pairs: three points on a line in either set, or a sample that does not keep its orientation
__device__ __forceinline__ bool hg_sample_ok(const double* x1, const double* y1, const double* x2, const double* y2) {
  const int TI[4] = {0, 0, 0, 1}, TJ[4] = {1, 1, 2, 2}, TK[4] = {2, 3, 3, 3};
  int negative = 0;
  bool ok = true;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int i = TI[t], j = TJ[t], k = TK[t];
#pragma unroll
    for (int set = 0; set < 2; ++set) {
      const double* x = set == 0 ? x1 : x2;
      const double* y = set == 0 ? y1 : y2;
      const double d1x = x[j] - x[i], d1y = y[j] - y[i], d2x = x[k] - x[i], d2y = y[k] - y[i];
      if (fabs(d1y * d2x - d1x * d2y) <= (double)FLT_EPSILON * (fabs(d1x) + fabs(d1y) + fabs(d2x) + fabs(d2y))) ok = false;
    }
    const double da = x1[i] * (y1[j] - y1[k]) - y1[i] * (x1[j] - x1[k]) + (x1[j] * y1[k] - y1[j] * x1[k]);
    const double db = x2[i] * (y2[j] - y2[k]) - y2[i] * (x2[j] - x2[k]) + (x2[j] * y2[k] - y2[j] * x2[k]);
    if (da * db < 0.0) ++negative;
  }
  return ok && (negative == 0 || negative == 4);
}

__global__ __launch_bounds__(RS_SOLVE_THREADS) void hg_solve_kernel(const double* __restrict__ pts1, const double* __restrict__ pts2,
                                                                    int n, int max_iters, uint64_t seed, double* __restrict__ Hc,
                                                                    int* __restrict__ count, double* __restrict__ hyp_H,
                                                                    int32_t* __restrict__ hyp_samples) {
  // per-thread LDS columns: sh[e * 64 + lane] (the elimination indexes rows and columns at run time)
  __shared__ double shA[72 * RS_SOLVE_THREADS];
  __shared__ int shI[(HG_MODEL + 8) * RS_SOLVE_THREADS];
  const int lane = threadIdx.x;
  const int it = blockIdx.x * RS_SOLVE_THREADS + lane;
  if (it >= max_iters) return;   // no workgroup barrier below
#define S_(k) shI[(k) * RS_SOLVE_THREADS + lane]
#define A_(r, c) shA[((r) * 9 + (c)) * RS_SOLVE_THREADS + lane]
  const int got = rs_sample<HG_MODEL>(seed, it, n, &shI[lane], RS_SOLVE_THREADS);
  if (hyp_samples) {
    for (int k = 0; k < HG_MODEL; ++k) hyp_samples[(size_t)it * HG_MODEL + k] = k < got ? S_(k) : -1;
  }
  bool ok = got == HG_MODEL;
  double H[9];
  if (ok) {
    // The sample's load and Hartley normalisation, rs_hartley<4> of ransac.h written out with checkSubset between the load
    // and the centroids: through rs_hartley the kernel took 132 registers instead of 104 and the call measured slower.
    double x1[HG_MODEL], y1[HG_MODEL], x2[HG_MODEL], y2[HG_MODEL];
    double c1x = 0.0, c1y = 0.0, c2x = 0.0, c2y = 0.0;
#pragma unroll
    for (int k = 0; k < HG_MODEL; ++k) {
      const int i = S_(k);
      x1[k] = f32r(pts1[(size_t)i * 2]);
      y1[k] = f32r(pts1[(size_t)i * 2 + 1]);
      x2[k] = f32r(pts2[(size_t)i * 2]);
      y2[k] = f32r(pts2[(size_t)i * 2 + 1]);
      c1x += x1[k], c1y += y1[k], c2x += x2[k], c2y += y2[k];
    }
    ok = hg_sample_ok(x1, y1, x2, y2);
    c1x /= HG_MODEL, c1y /= HG_MODEL, c2x /= HG_MODEL, c2y /= HG_MODEL;
    double m1 = 0.0, m2 = 0.0;
#pragma unroll
    for (int k = 0; k < HG_MODEL; ++k) {
      const double ax = x1[k] - c1x, ay = y1[k] - c1y, bx = x2[k] - c2x, by = y2[k] - c2y;
      m1 += sqrt(ax * ax + ay * ay);
      m2 += sqrt(bx * bx + by * by);
    }
    m1 /= HG_MODEL, m2 /= HG_MODEL;
    ok = ok && m1 > 0.0 && m2 > 0.0 && m1 < INFINITY && m2 < INFINITY;
    const double s1 = M_SQRT2 / m1, s2 = M_SQRT2 / m2;
    if (ok) {
      // rows [x, y, 1, 0, 0, 0, -xu, -yu | u] (k) and [0, 0, 0, x, y, 1, -xv, -yv | v] (k + 4) in normalised coordinates
#pragma unroll
      for (int k = 0; k < HG_MODEL; ++k) {
        const double x = (x1[k] - c1x) * s1, y = (y1[k] - c1y) * s1;
        const double u = (x2[k] - c2x) * s2, v = (y2[k] - c2y) * s2;
        A_(k, 0) = x, A_(k, 1) = y, A_(k, 2) = 1.0, A_(k, 3) = 0.0, A_(k, 4) = 0.0, A_(k, 5) = 0.0;
        A_(k, 6) = -(x * u), A_(k, 7) = -(y * u), A_(k, 8) = u;
        A_(k + 4, 0) = 0.0, A_(k + 4, 1) = 0.0, A_(k + 4, 2) = 0.0, A_(k + 4, 3) = x, A_(k + 4, 4) = y, A_(k + 4, 5) = 1.0;
        A_(k + 4, 6) = -(x * v), A_(k + 4, 7) = -(y * v), A_(k + 4, 8) = v;
      }
      double hn[9];
      ok = rs_solve<8, RS_SOLVE_THREADS>(&shA[lane], &shI[HG_MODEL * RS_SOLVE_THREADS + lane], hn);
      if (ok) {
        hn[8] = 1.0;
        hg_denormalise(hn, c1x, c1y, s1, c2x, c2y, s2, H);
        rs_scale9(H);
      }
    }
  }
#undef S_
#undef A_
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const double v = ok ? H[i] : NAN;   // a slot without a candidate: NaN, count -1
    Hc[(size_t)it * 9 + i] = v;
    if (hyp_H) hyp_H[(size_t)it * 9 + i] = v;
  }
  count[it] = ok ? 0 : -1;
}

// ---- the refit -----------------------------------------------------------------------------------------------------
// One inlier's terms, added to acc: every stage reads the point rounded to float32.
template <int STAGE>
__device__ __forceinline__ void hg_terms(const HgState* __restrict__ st, double x, double y, double u, double v, double* acc) {
  if (STAGE == HG_CENTROID) {
    acc[0] += x, acc[1] += y, acc[2] += u, acc[3] += v, acc[4] += 1.0;
    return;
  }
  const double ax = x - st->c1x, ay = y - st->c1y, bx = u - st->c2x, by = v - st->c2y;
  if (STAGE == HG_DISTANCE) {
    acc[0] += sqrt(ax * ax + ay * ay);
    acc[1] += sqrt(bx * bx + by * by);
    return;
  }
  const double X = ax * st->s1, Y = ay * st->s1, U = bx * st->s2, V = by * st->s2;
  if (STAGE == HG_DLT) {
    const double r1[9] = {X, Y, 1.0, 0.0, 0.0, 0.0, -(U * X), -(U * Y), -U};
    const double r2[9] = {0.0, 0.0, 0.0, X, Y, 1.0, -(V * X), -(V * Y), -V};
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
      for (int j = i; j < 9; ++j) acc[rf_tri<9>(i, j)] += r1[i] * r1[j] + r2[i] * r2[j];
    return;
  }
  // HG_GN: residual and Jacobian of the 8 free entries at st->h (h[8] = 1)
  const double* h = st->h;
  const double w = 1.0 / (h[6] * X + h[7] * Y + h[8]);
  const double px = (h[0] * X + h[1] * Y + h[2]) * w, py = (h[3] * X + h[4] * Y + h[5]) * w;
  const double rx = px - U, ry = py - V;
  const double xw = X * w, yw = Y * w;
  const double j1[8] = {xw, yw, w, 0.0, 0.0, 0.0, -(xw * px), -(yw * px)};
  const double j2[8] = {0.0, 0.0, 0.0, xw, yw, w, -(xw * py), -(yw * py)};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
#pragma unroll
    for (int j = i; j < 8; ++j) acc[rf_tri<8>(i, j)] += j1[i] * j1[j] + j2[i] * j2[j];
    acc[36 + i] += j1[i] * rx + j2[i] * ry;
  }
  acc[44] += rx * rx + ry * ry;
}

template <int STAGE>
struct HgTerms {
  static constexpr int SUMS = STAGE == HG_CENTROID ? 5 : STAGE == HG_DISTANCE ? 2 : HG_SUMS, STRIDE = HG_SUMS;
  using Points = RsPixelPairs;
  using State = HgState;
  static __device__ __forceinline__ void terms(const HgState* __restrict__ st, const Points& pts, int p, double* acc) {
    const double x = f32r(pts.pts1[(size_t)p * 2]), y = f32r(pts.pts1[(size_t)p * 2 + 1]);
    const double u = f32r(pts.pts2[(size_t)p * 2]), v = f32r(pts.pts2[(size_t)p * 2 + 1]);
    hg_terms<STAGE>(st, x, y, u, v, acc);
  }
};

// the eigenvector of the smallest eigenvalue of the symmetric 9 x 9 a (destroyed), by cyclic Jacobi (ransac.h) -> e[9]
__device__ void hg_jacobi9(double (*a)[9], double (*v)[9], double* e) {
  rs_jacobi<9>(a, v);
  int m = 0;
  for (int i = 1; i < 9; ++i)
    if (a[i][i] < a[m][m]) m = i;
  for (int i = 0; i < 9; ++i) e[i] = v[i][m];
}

// stage: which sums the accumulate before it made;
// last: the chain's last launch (no further step is taken; writes H_out and info[4..7])
__global__ __launch_bounds__(64) void hg_finish_kernel(int chunks, const double* __restrict__ parts, HgState* __restrict__ st, int stage,
                                                       int last, const double* __restrict__ Hc, double* __restrict__ H_out,
                                                       int32_t* __restrict__ info) {
  __shared__ double sums[HG_SUMS];
  __shared__ double A[9][9], Vv[9][9];
  const bool active = !st->done;   // uniform; read before anything below writes it
  const int ns = stage == HG_CENTROID ? 5 : stage == HG_DISTANCE ? 2 : HG_SUMS;
  rf_reduce<HG_SUMS>(parts, chunks, active ? ns : 0, sums);
  if (threadIdx.x != 0) return;
  if (active) {
    if (stage == HG_CENTROID) {
      const double cnt = sums[4];
      st->cnt = cnt;
      st->c1x = sums[0] / cnt, st->c1y = sums[1] / cnt, st->c2x = sums[2] / cnt, st->c2y = sums[3] / cnt;
    } else if (stage == HG_DISTANCE) {
      const double m1 = sums[0] / st->cnt, m2 = sums[1] / st->cnt;
      if (m1 > 0.0 && m2 > 0.0 && m1 < INFINITY && m2 < INFINITY) {
        st->s1 = M_SQRT2 / m1, st->s2 = M_SQRT2 / m2;
      } else {
        st->done = 1;   // status stays 2: no refit
      }
    } else if (stage == HG_DLT) {
      for (int i = 0; i < 9; ++i)
        for (int j = i; j < 9; ++j) A[i][j] = A[j][i] = sums[rf_tri<9>(i, j)];
      double e[9];
      hg_jacobi9(A, Vv, e);
      double ss = 0.0;
      bool finite = true;
      for (int i = 0; i < 9; ++i) ss += e[i] * e[i], finite = finite && isfinite(e[i]);
      if (!finite || !(ss > 0.0)) {
        st->done = 1;   // status stays 2
      } else {
        const bool refine = fabs(e[8]) > HG_H22_TOL * sqrt(ss);
        for (int i = 0; i < 9; ++i) st->h[i] = refine ? e[i] / e[8] : e[i];
        if (refine) st->h[8] = 1.0;
        st->status = 1;
        st->trial = 0;
        if (!refine || last) st->done = 1;
      }
    } else {   // HG_GN
      rf_step(st, sums, last);
    }
  }
  if (last) {
    const int found = info[0], status = st->status;
    double H[9];
    if (!found) {
      for (int i = 0; i < 9; ++i) H[i] = 0.0;
    } else if (status == 2) {
      for (int i = 0; i < 9; ++i) H[i] = Hc[(size_t)info[3] * 9 + i];
    } else {
      hg_denormalise(st->h, st->c1x, st->c1y, st->s1, st->c2x, st->c2y, st->s2, H);
      rs_scale9(H);
    }
    for (int i = 0; i < 9; ++i) H_out[i] = H[i];
    info[4] = st->kept;
    info[5] = status;
    info[6] = 0;
    info[7] = 0;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------
namespace {

const RsEntry HG_ENTRY = {"cotr_ransac_homography", "H_out", HG_MODEL, "", HgModel::SLOTS, RS_MAX_ITERS};

// after the frame's candidates and counts: the refit's state, then its partial sums [chunks, HG_SUMS]
RfPlan hg_plan(const RsPlan& rs, int n) { return rf_plan(rs.bytes, sizeof(HgState), n, HG_SUMS); }

}  // namespace

extern "C" {

int cotr_ransac_homography_scratch_bytes(int n, int max_iters, size_t* bytes) {
  if (const int rc = rs_scratch_bytes(HG_ENTRY, n, max_iters, bytes)) return rc;
  *bytes = hg_plan(rs_plan(HG_ENTRY, max_iters), n).bytes;
  return COTR_OK;
}

int cotr_ransac_homography(const double* pts1, const double* pts2, int n, double threshold, double confidence, int max_iters,
                           int refine_iters, uint64_t seed, double* H_out, uint8_t* mask_out, int32_t* info_out, double* H_ransac,
                           double* hyp_H, int32_t* hyp_count, int32_t* hyp_samples, void* scratch, size_t scratch_bytes,
                           cotr_stream stream) {
  const RsPlan rs = rs_plan(HG_ENTRY, max_iters);
  const RfPlan l = hg_plan(rs, n);
  if (const int rc = rs_check_call(HG_ENTRY, n, max_iters, threshold, confidence, pts1, pts2, H_out, mask_out, info_out, hyp_H, hyp_count,
                                   hyp_samples, scratch, scratch_bytes, l.bytes))
    return rc;
  if (refine_iters < 0 || refine_iters > HG_MAX_REFINE) return rs_fail(HG_ENTRY, "refine_iters must be in [0, 64]");
  if (!aligned(H_ransac, 8)) return rs_fail(HG_ENTRY, "H_ransac must be 8-byte aligned");
  char* base = static_cast<char*>(scratch);
  const double* Hc = reinterpret_cast<const double*>(base + rs.candidates);
  HgState* st = reinterpret_cast<HgState*>(base + l.state);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const auto solve = [&](double* cand, int* count) {
    hipLaunchKernelGGL(hg_solve_kernel, dim3((unsigned)((max_iters + RS_SOLVE_THREADS - 1) / RS_SOLVE_THREADS)), dim3(RS_SOLVE_THREADS), 0, s,
                       pts1, pts2, n, max_iters, seed, cand, count, hyp_H, hyp_samples);
  };
  rs_enqueue<HgModel>(s, solve, {pts1, pts2}, n, max_iters, confidence, (float)(threshold * threshold), rs, scratch, H_ransac, mask_out,
                      info_out, hyp_count, {st});
  const RsPixelPairs pts = {pts1, pts2};
  const auto pair = [&](auto terms, int stage, int last) {
    rf_enqueue_pair<decltype(terms)>(s, l, scratch, pts, n, mask_out, hg_finish_kernel, stage, last, Hc, H_out, info_out);
  };
  pair(HgTerms<HG_CENTROID>(), HG_CENTROID, 0);
  pair(HgTerms<HG_DISTANCE>(), HG_DISTANCE, 0);
  // refine_iters = 0: the DLT's finish is the last launch (status 1); else pair j judges step j - 1 and takes step j
  pair(HgTerms<HG_DLT>(), HG_DLT, refine_iters == 0);
  for (int j = 0; refine_iters > 0 && j <= refine_iters; ++j) pair(HgTerms<HG_GN>(), HG_GN, j == refine_iters);
  return launched();
}
}  // extern "C"
