// The frame of the RANSAC estimators (guided.hip: fundamental matrix, homography.hip: homography, essential.hip: essential
// matrix, pnp.hip: absolute pose, rigid3d.hip: 3D-3D registration).  A model is a struct M with
//   MODEL, SLOTS      sample size, candidate slots per iteration (slot = SLOTS * it + k)
//   Points            what its kernels read the correspondences from, passed to them by value
//   inlier(m, pts, p, thr)   whether point p is an inlier of the candidate m[9]
//   Tail, tail(t, found)     what thread 0 of the mask kernel does besides, with its arguments
// and a solve kernel of its own that fills the SLOTS * max_iters slots (a slot without a candidate: NaN, count -1).  Shared
// here: the counter-based sampler, the wavefront sum of the refits (refit.h), the sample's Hartley normalisation, the
// full-pivot elimination with its solve and null-vector forms, the scaling rule of a 3 x 3 result, rs_count_kernel<M>,
// OpenCV's iteration update, the kernel that
// replays the sequential selection loop on the counts, rs_mask_kernel<M>, the cyclic Jacobi iteration of the symmetric
// eigenproblems, and on the host the scratch prefix, the argument checks and the launch sequence.  Rules in DESIGN.md 3h.
// Included by translation units compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "handleless.h"

#define RS_HD __host__ __device__
#define RS_MAX_DRAWS 64
#define RS_SOLVE_THREADS 64
#define RS_COUNT_THREADS 256
#define RS_COUNT_STEPS 8       // points per thread per workgroup: chunks of 2048 points
#define RS_CHUNK (RS_COUNT_THREADS * RS_COUNT_STEPS)
#define RS_SELECT_THREADS 1024
#define RS_MAX_ITERS (1 << 16)
#define RS_MAX_POINTS (1 << 24)
#define RS_RANK_TOL 1e-12      // a pivot below this times the first one: the sample is degenerate
#define RS_JACOBI_SWEEPS 30

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ double f32r(double v) { return (double)(float)v; }

// the sum over a wavefront by a fixed butterfly: every lane ends with the same bits
__device__ __forceinline__ double rs_wave_sum(double a) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a = a + __shfl_xor(a, off);
  return a;
}

// Sample of iteration it: draw d is splitmix64(splitmix64(seed) ^ (it << 6 | d)), index (z >> 32) % n; duplicates are
// rejected; the first MODEL distinct indices of at most RS_MAX_DRAWS draws go to s[k * stride].  Returns how many it got.
template <int MODEL>
__device__ __forceinline__ int rs_sample(uint64_t seed, int it, int n, int* s, int stride) {
  const uint64_t sk = splitmix64(seed);
  int got = 0;
  for (int d = 0; d < RS_MAX_DRAWS && got < MODEL; ++d) {
    const uint64_t z = splitmix64(sk ^ (((uint64_t)it << 6) | (uint64_t)d));
    const int c = (int)((z >> 32) % (uint64_t)n);
    bool dup = false;
    for (int k = 0; k < got; ++k) dup = dup || s[k * stride] == c;
    if (!dup) {
      s[got * stride] = c;
      ++got;
    }
  }
  return got;
}

// The pixel pairs of a sample, rounded to float32, and their Hartley normalisation T = [[s, 0, -s cx], [0, s, -s cy],
// [0, 0, 1]] per point set: c the centroid, s = sqrt 2 over the mean distance to it.
template <int MODEL>
struct RsHartley {
  double x1[MODEL], y1[MODEL], x2[MODEL], y2[MODEL];
  double c1x, c1y, s1, c2x, c2y, s2;
};

// the sample s[k * stride] of pts1 -> pts2; false when a mean distance is 0 or not finite
template <int MODEL>
__device__ __forceinline__ bool rs_hartley(const double* __restrict__ pts1, const double* __restrict__ pts2, const int* s, int stride,
                                           RsHartley<MODEL>& h) {
  double c1x = 0.0, c1y = 0.0, c2x = 0.0, c2y = 0.0;
#pragma unroll
  for (int k = 0; k < MODEL; ++k) {
    const int i = s[k * stride];
    h.x1[k] = f32r(pts1[(size_t)i * 2]);
    h.y1[k] = f32r(pts1[(size_t)i * 2 + 1]);
    h.x2[k] = f32r(pts2[(size_t)i * 2]);
    h.y2[k] = f32r(pts2[(size_t)i * 2 + 1]);
    c1x += h.x1[k], c1y += h.y1[k], c2x += h.x2[k], c2y += h.y2[k];
  }
  c1x /= MODEL, c1y /= MODEL, c2x /= MODEL, c2y /= MODEL;
  double m1 = 0.0, m2 = 0.0;
#pragma unroll
  for (int k = 0; k < MODEL; ++k) {
    const double ax = h.x1[k] - c1x, ay = h.y1[k] - c1y, bx = h.x2[k] - c2x, by = h.y2[k] - c2y;
    m1 += sqrt(ax * ax + ay * ay);
    m2 += sqrt(bx * bx + by * by);
  }
  m1 /= MODEL, m2 /= MODEL;
  h.c1x = c1x, h.c1y = c1y, h.c2x = c2x, h.c2y = c2y;
  h.s1 = M_SQRT2 / m1, h.s2 = M_SQRT2 / m2;
  return m1 > 0.0 && m2 > 0.0 && m1 < INFINITY && m2 < INFINITY;
}

// ---- full-pivot elimination ---------------------------------------------------------------------------------------------
// a: ROWS x COLS, entry (r, c) at a[(r * COLS + c) * STRIDE]; perm: PCOLS ints at perm[c * STRIDE].  ROWS pivot steps: step k
// takes the first entry of largest magnitude of rows [k, ROWS) x columns [k, PCOLS) (a NaN entry is passed over), swaps its
// row and its column (and perm) into place and eliminates column k below it, over the columns [k + 1, COLS).  false when a
// pivot is not above RS_RANK_TOL times the first one (or is NaN): the system is degenerate.
template <int ROWS, int PCOLS, int COLS, int STRIDE>
RS_HD bool rs_eliminate(double* a, int* perm) {
#define RS_A_(r, c) a[((r) * COLS + (c)) * STRIDE]
#define RS_P_(c) perm[(c) * STRIDE]
  for (int c = 0; c < PCOLS; ++c) RS_P_(c) = c;
  double piv0 = 0.0;
  for (int k = 0; k < ROWS; ++k) {
    double pv = -1.0;
    int pr = k, pc = k;
    for (int r = k; r < ROWS; ++r)
      for (int c = k; c < PCOLS; ++c) {
        const double v = fabs(RS_A_(r, c));
        if (v > pv) pv = v, pr = r, pc = c;
      }
    if (k == 0) piv0 = pv;
    if (!(pv > RS_RANK_TOL * piv0)) return false;   // also for NaN
    if (pr != k)
      for (int c = 0; c < COLS; ++c) {
        const double t = RS_A_(k, c);
        RS_A_(k, c) = RS_A_(pr, c);
        RS_A_(pr, c) = t;
      }
    if (pc != k) {
      for (int r = 0; r < ROWS; ++r) {
        const double t = RS_A_(r, k);
        RS_A_(r, k) = RS_A_(r, pc);
        RS_A_(r, pc) = t;
      }
      const int t = RS_P_(k);
      RS_P_(k) = RS_P_(pc);
      RS_P_(pc) = t;
    }
    const double akk = RS_A_(k, k);
    for (int r = k + 1; r < ROWS; ++r) {
      const double m = RS_A_(r, k) / akk;
      for (int c = k + 1; c < COLS; ++c) RS_A_(r, c) = RS_A_(r, c) - m * RS_A_(k, c);
      RS_A_(r, k) = 0.0;
    }
  }
  return true;
}

// a: the augmented N x (N + 1) system -> z[N] with A z = b; false when it is degenerate
template <int N, int STRIDE>
RS_HD bool rs_solve(double* a, int* perm, double* z) {
  constexpr int COLS = N + 1;
  if (!rs_eliminate<N, N, COLS, STRIDE>(a, perm)) return false;
  double y[N];
#pragma unroll
  for (int r = N - 1; r >= 0; --r) {
    double acc = RS_A_(r, N);
#pragma unroll
    for (int c = r + 1; c < N; ++c) acc -= RS_A_(r, c) * y[c];
    y[r] = acc / RS_A_(r, r);
  }
  // z[perm[c]] = y[c], without indexing registers at run time
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double v = 0.0;
#pragma unroll
    for (int c = 0; c < N; ++c) v = RS_P_(c) == i ? y[c] : v;
    z[i] = v;
  }
  return true;
}

// After rs_eliminate<ROWS, COLS, COLS>: the null vector with the free (permuted) column `one` set to 1 and the other free
// columns to 0, by back substitution -> z[COLS] in permuted order (entry c belongs to column perm[c]).
template <int ROWS, int COLS, int STRIDE>
RS_HD __forceinline__ void rs_null_vector(const double* a, int one, double* z) {
#pragma unroll
  for (int c = ROWS; c < COLS; ++c) z[c] = c == one ? 1.0 : 0.0;
#pragma unroll
  for (int r = ROWS - 1; r >= 0; --r) {
    double acc = 0.0;
#pragma unroll
    for (int c = r + 1; c < COLS; ++c) acc += RS_A_(r, c) * z[c];
    z[r] = -acc / RS_A_(r, r);
  }
}
#undef RS_A_
#undef RS_P_

// ---- the scale of a 3 x 3 result ------------------------------------------------------------------------------------------
// whether the first entry of largest magnitude is negative (the result is then negated: that entry made positive)
RS_HD __forceinline__ bool rs_negative9(const double* m) {
  double big = m[0];
#pragma unroll
  for (int i = 1; i < 9; ++i)
    if (fabs(m[i]) > fabs(big)) big = m[i];
  return big < 0.0;
}

// unit Frobenius norm, then m[2,2] = 1 unless |m[2,2]| <= DBL_EPSILON (then: negated if rs_negative9)
RS_HD __forceinline__ void rs_scale9(double* m) {
  double ss = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) ss += m[i] * m[i];
  const double nrm = sqrt(ss);
#pragma unroll
  for (int i = 0; i < 9; ++i) m[i] = m[i] / nrm;
  if (fabs(m[8]) > DBL_EPSILON) {
    const double m22 = m[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) m[i] = m[i] / m22;
    m[8] = 1.0;
  } else if (rs_negative9(m)) {
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = -m[i];
  }
}

// pts1 -> pts2 in pixels: the Points of the fundamental-matrix and homography models
struct RsPixelPairs {
  const double* __restrict__ pts1;
  const double* __restrict__ pts2;
};

// ---- counting -------------------------------------------------------------------------------------------------------------
// grid (SLOTS * max_iters slots) x (RS_CHUNK-point chunks): ballot + popcount per wavefront, one integer atomicAdd per
// wavefront (integer sums: deterministic)
template <class M>
__global__ __launch_bounds__(RS_COUNT_THREADS) void rs_count_kernel(typename M::Points pts, int n, const double* __restrict__ cand,
                                                                    int* __restrict__ count, float thr) {
  const int slot = blockIdx.x;
  if (count[slot] < 0) return;   // no candidate in this slot (uniform)
  double m[9];
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    m[i] = cand[(size_t)slot * 9 + i];
    finite = finite && isfinite(m[i]);
  }
  if (!finite) return;           // a non-finite candidate counts 0 inliers
  const int base = blockIdx.y * RS_CHUNK;
  int wc = 0;
#pragma unroll
  for (int s = 0; s < RS_COUNT_STEPS; ++s) {
    const int p = base + s * RS_COUNT_THREADS + threadIdx.x;
    const bool in = p < n && M::inlier(m, pts, p, thr);
    wc += __popcll(__ballot(in));
  }
  if ((threadIdx.x & 63) == 0 && wc > 0) atomicAdd(&count[slot], wc);
}

// OpenCV's RANSACUpdateNumIters
__device__ inline int ransac_update(double p, double ep, int m, int N) {
  const double num = log(fmax(1.0 - p, DBL_MIN));
  const double denom = 1.0 - pow(1.0 - ep, (double)m);
  if (denom < DBL_MIN) return 0;
  const double lden = log(denom);
  return (lden >= 0.0 || -num >= (double)N * (-lden)) ? N : (int)rint(num / lden);
}

// Cyclic Jacobi on the symmetric N x N a: rotations (p, q) in row-major order until the off-diagonal norm falls below
// DBL_EPSILON times the Frobenius norm, at most RS_JACOBI_SWEEPS sweeps.  a ends (nearly) diagonal with the eigenvalues, the
// columns of v are the eigenvectors.  One thread.
template <int N>
__device__ void rs_jacobi(double (*a)[N], double (*v)[N]) {
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) v[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < RS_JACOBI_SWEEPS; ++sweep) {
    double off = 0.0, all = 0.0;
    for (int i = 0; i < N; ++i)
      for (int j = 0; j < N; ++j) {
        const double t = a[i][j] * a[i][j];
        all += t;
        if (i != j) off += t;
      }
    if (!(sqrt(off) >= DBL_EPSILON * sqrt(all))) break;   // converged (or NaN)
    for (int p = 0; p < N - 1; ++p)
      for (int q = p + 1; q < N; ++q) {
        const double apq = a[p][q];
        if (apq == 0.0) continue;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
        const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < N; ++k) {   // columns p and q
          const double akp = a[k][p], akq = a[k][q];
          a[k][p] = c * akp - s * akq;
          a[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < N; ++k) {   // rows p and q
          const double apk = a[p][k], aqk = a[q][k];
          a[p][k] = c * apk - s * aqk;
          a[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < N; ++k) {
          const double vkp = v[k][p], vkq = v[k][q];
          v[k][p] = c * vkp - s * vkq;
          v[k][q] = s * vkp + c * vkq;
        }
      }
  }
}

// The sequential loop, replayed: the next slot that beats max(best, MODEL - 1) within the iterations still to run is found
// by a parallel minimum over the slots after the last one taken.  SLOTS candidates per iteration (slot = SLOTS * it + k).
// info = {found, best, iterations run, chosen slot}.
template <int MODEL, int SLOTS>
__global__ __launch_bounds__(RS_SELECT_THREADS) void rs_select_kernel(const int* __restrict__ count, int max_iters, int n, double confidence,
                                                                      int32_t* __restrict__ info, int32_t* __restrict__ hyp_count) {
  __shared__ int st[4];   // next slot to look at (-1: done), best, niters, chosen slot
  __shared__ int red[RS_SELECT_THREADS / 64];
  const int tid = threadIdx.x;
  const int nslots = SLOTS * max_iters;
  if (hyp_count)
    for (int s = tid; s < nslots; s += RS_SELECT_THREADS) hyp_count[s] = count[s];
  if (tid == 0) st[0] = 0, st[1] = 0, st[2] = max_iters, st[3] = -1;
  __syncthreads();
  for (;;) {
    const int pos = st[0], best = st[1], niters = st[2], chosen = st[3];
    if (pos < 0) break;   // uniform
    const int thr = max(best, MODEL - 1);
    // slots of the iterations it < niters, and the rest of the iteration of the last slot taken
    const int limit = SLOTS * max(niters, chosen >= 0 ? chosen / SLOTS + 1 : 0);
    int local = INT_MAX;
    for (int s = pos + tid; s < limit; s += RS_SELECT_THREADS)
      if (count[s] > thr) {
        local = s;
        break;
      }
    for (int off = 32; off > 0; off >>= 1) local = min(local, __shfl_xor(local, off));
    if ((tid & 63) == 0) red[tid >> 6] = local;
    __syncthreads();
    if (tid == 0) {
      int m = INT_MAX;
      for (int w = 0; w < RS_SELECT_THREADS / 64; ++w) m = min(m, red[w]);
      if (m == INT_MAX) {
        st[0] = -1;
      } else {
        const int nb = count[m];
        st[0] = m + 1;
        st[1] = nb;
        st[2] = ransac_update(confidence, (double)(n - nb) / (double)n, MODEL, niters);
        st[3] = m;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int chosen = st[3];
    info[0] = chosen >= 0 ? 1 : 0;
    info[1] = st[1];
    info[2] = chosen >= 0 ? max(st[2], chosen / SLOTS + 1) : max_iters;
    info[3] = chosen;
  }
}

// The chosen candidate -> out (zeros when nothing was found; out may be NULL) and its mask, by the count kernel's predicate.
// A chosen slot is finite: its count is above MODEL - 1, and a non-finite candidate counts 0.  Thread 0 runs the model's tail.
template <class M>
__global__ __launch_bounds__(256) void rs_mask_kernel(typename M::Points pts, int n, const double* __restrict__ cand,
                                                      const int32_t* __restrict__ info, float thr, double* __restrict__ out,
                                                      uint8_t* __restrict__ mask, typename M::Tail tail) {
  const int found = info[0], slot = info[3];
  const int p = blockIdx.x * 256 + threadIdx.x;
  double m[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) m[i] = found ? cand[(size_t)slot * 9 + i] : 0.0;
  if (p < n) mask[p] = (found && M::inlier(m, pts, p, thr)) ? 1 : 0;
  if (p < 9 && out) out[p] = found ? cand[(size_t)slot * 9 + p] : 0.0;
  if (p == 0) M::tail(tail, found);
}

// ---- host side ------------------------------------------------------------------------------------------------------------
namespace cotr_detail {

// what an estimator's entry points tell the shared checks: their name and their model argument's (F_out, ...), the fewest
// correspondences (with a note for the message about them, "" for none), the candidate slots per iteration and the most
// iterations
struct RsEntry {
  const char* name;
  const char* model_out;
  int least;
  const char* note;
  int slots;
  int max_iters;
};

// the start of every estimator's scratch: the candidates [slots, 9] and their counts [slots]; a model's own regions follow
// from `bytes`
struct RsPlan {
  size_t candidates, counts, bytes;
};

inline RsPlan rs_plan(const RsEntry& e, int max_iters) {
  RsPlan l;
  const size_t slots = (size_t)e.slots * max_iters;
  l.candidates = 0;
  l.counts = align_up(slots * 9 * sizeof(double));
  l.bytes = l.counts + align_up(slots * sizeof(int));
  return l;
}

inline int rs_fail(const RsEntry& e, const char* what, const char* note = "") { return arg_fail(e.name, what, note); }

inline int rs_check_shape(const RsEntry& e, int n, int max_iters) {
  char what[64];
  if (n < e.least || n > RS_MAX_POINTS) {
    snprintf(what, sizeof what, "n must be in [%d, 2^24]", e.least);
    return rs_fail(e, what, e.note);
  }
  if (max_iters < 1 || max_iters > e.max_iters) {
    snprintf(what, sizeof what, "max_iters must be in [1, %d]", e.max_iters);
    return rs_fail(e, what);
  }
  return COTR_OK;
}

// the checks of a *_scratch_bytes entry point -> the bytes of the shared prefix
inline int rs_scratch_bytes(const RsEntry& e, int n, int max_iters, size_t* bytes) {
  if (!bytes) return rs_fail(e, "bytes is NULL");
  if (const int rc = rs_check_shape(e, n, max_iters)) return rc;
  *bytes = rs_plan(e, max_iters).bytes;
  return COTR_OK;
}

// the arguments every estimator takes; `need`: the scratch size of the call
inline int rs_check_call(const RsEntry& e, int n, int max_iters, double threshold, double confidence, const double* pts1, const double* pts2,
                         const double* model_out, const uint8_t* mask_out, const int32_t* info_out, const double* hyp_model,
                         const int32_t* hyp_count, const int32_t* hyp_samples, const void* scratch, size_t scratch_bytes, size_t need) {
  if (const int rc = rs_check_shape(e, n, max_iters)) return rc;
  if (!(threshold > 0.0) || !(threshold < INFINITY)) return rs_fail(e, "threshold must be finite and > 0");
  if (!(confidence > 0.0 && confidence < 1.0)) return rs_fail(e, "confidence must be in (0, 1)");
  if (!pts1 || !pts2 || !model_out || !mask_out || !info_out || !scratch) {
    char what[96];
    snprintf(what, sizeof what, "pts1, pts2, %s, mask_out, info_out and scratch must not be NULL", e.model_out);
    return rs_fail(e, what);
  }
  if (!aligned(pts1, 8) || !aligned(pts2, 8) || !aligned(model_out, 8) || !aligned(info_out, 4) || !aligned(hyp_model, 8) ||
      !aligned(hyp_count, 4) || !aligned(hyp_samples, 4) || !aligned(scratch, 16))
    return rs_fail(e, "doubles must be 8-byte, ints 4-byte and scratch 16-byte aligned");
  if (scratch_bytes < need) return rs_fail(e, "scratch is smaller than its _scratch_bytes function returns");
  return COTR_OK;
}

// solve -> count -> select -> mask of model M on stream s; launch_solve(candidates, counts) launches the model's solve kernel
template <class M, class LaunchSolve>
inline void rs_enqueue(hipStream_t s, LaunchSolve launch_solve, const typename M::Points& pts, int n, int max_iters, double confidence,
                       float thr, const RsPlan& l, void* scratch, double* model_out, uint8_t* mask_out, int32_t* info_out,
                       int32_t* hyp_count, const typename M::Tail& tail) {
  double* cand = reinterpret_cast<double*>(static_cast<char*>(scratch) + l.candidates);
  int* count = reinterpret_cast<int*>(static_cast<char*>(scratch) + l.counts);
  launch_solve(cand, count);
  hipLaunchKernelGGL(rs_count_kernel<M>, dim3((unsigned)(M::SLOTS * max_iters), (unsigned)((n + RS_CHUNK - 1) / RS_CHUNK)), dim3(RS_COUNT_THREADS), 0,
                     s, pts, n, cand, count, thr);
  hipLaunchKernelGGL((rs_select_kernel<M::MODEL, M::SLOTS>), dim3(1), dim3(RS_SELECT_THREADS), 0, s, count, max_iters, n, confidence, info_out,
                     hyp_count);
  hipLaunchKernelGGL(rs_mask_kernel<M>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pts, n, cand, info_out, thr, model_out, mask_out, tail);
}

}  // namespace cotr_detail
