// Bundle adjustment: cotr_bundle_adjust, Levenberg-Marquardt on the summed squared pixel error over the poses of the free views
// and the points together, by the Schur complement of the points.  Handle-less (handleless.h), stream-ordered,
// integer atomics only, every floating-point sum in a fixed order: the same input gives the same bits.  Compiled with
// -ffp-contract=off.  The view table, the pixel, the projection and the cofactor rule are those of structure.hip (view_table.h).
//
//   tv_prepare_kernel  the view table of the input poses (view_table.h); info[0] = found
//   ba_init_kernel     the counters zeroed, the state set: buffer 0 current, no step taken
//   per round:
//     ba_count_kernel     a thread per point: the round's set before the starved views leave it, observations per view counted
//     ba_classify_kernel  the frozen views' observations leave the set, landmarks marked, used_out, the cost of the set per workgroup
//     ba_begin_kernel     one wavefront sums the cost, then one thread: lambda = lambda0, the free views and their slots in the reduced system
//     per iteration:
//       ba_points_kernel  a thread per point: V_p, g_p, the damped inverse and V_p*^-1 g_p -> 9 doubles per point
//       ba_pairs_kernel   (view pair v <= w) x (chunk): the sums of W_v V*^-1 W_w^T, on the diagonal also U_v and b_v, per chunk
//       ba_solve_kernel   one workgroup: the chunks in order, S and b assembled in LDS, Cholesky and both solves (chol.h), the candidate poses
//       ba_update_kernel  a thread per point: the candidate X, its squared error and depth flag over the set, per workgroup
//       ba_decide_kernel  one wavefront sums the cost, then one thread keeps or rejects the candidate (the current-buffer index flips), lambda, the counters
//   ba_finish_kernel   the outputs
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "chol.h"
#include "handleless.h"
#include "ransac.h"
#include "rodrigues.h"
#include "view_table.h"

using namespace cotr_detail;

#define BA_MAX_POINTS (1 << 20)
#define BA_MAX_ROUNDS 8
#define BA_MAX_ITERS 64
#define BA_THREADS 256
#define BA_MIN_VIEW_OBS 4
#define BA_MAX_DIM (6 * (TV_MAX_VIEWS - 1))   // 186 unknowns of the reduced system
#define BA_TAB (TV_MAX_VIEWS * TV_ROW)
// the sums of a view pair per chunk: Y = W_v V*^-1 W_w^T (36, row-major) | U_v (21, upper triangle by rows) | b_v (6) | unused
#define BA_SUMS 64
#define BA_U 36
#define BA_B 57
#define BA_NSUMS 63
#define BA_LAMBDA_MIN 1e-12
#define BA_LAMBDA_MAX 1e12

struct BaState {
  double lambda, cost, cost_first;
  int cur, done, bad, found;
  int F, nobs, nfrozen, nlandmarks, kept, rejected, rounds_run;
  uint32_t free_mask;
  int slot[TV_MAX_VIEWS];   // the place of a free view among the free views, -1 otherwise
};

// integer counters: observations per view and round | observations per round | landmarks per round | candidates behind a camera
#define BA_CNT_OBS (BA_MAX_ROUNDS * TV_MAX_VIEWS)
#define BA_CNT_LM (BA_CNT_OBS + BA_MAX_ROUNDS)
#define BA_CNT_BEHIND (BA_CNT_LM + BA_MAX_ROUNDS)
#define BA_COUNTERS (BA_CNT_BEHIND + 1)

struct BaScratch {
  double* tab;      // [2][BA_TAB] the view tables of the two state buffers
  BaState* st;
  int* cnt;         // [BA_COUNTERS]
  double* dc;       // [192] the step of the free views
  double* X;        // [2][n][3]
  uint32_t* set;    // [n] the views of the round's set per point
  uint8_t* lm;      // [n] landmark of the round
  uint8_t* moves;   // [n] the point takes a step in this iteration
  double* pt;       // [n][9] V*^-1 (00 01 02 11 12 22) | V*^-1 g
  double* cparts;   // [ceil(n / 256)] cost per workgroup of ba_classify_kernel / ba_update_kernel
  double* parts;    // [pairs][chunks][BA_SUMS]
  size_t bytes;
};

static BaScratch ba_layout(void* base, int V, int n) {
  BaScratch l;
  const size_t N = (size_t)n, chunks = (N + RS_CHUNK - 1) / RS_CHUNK, pairs = (size_t)V * (V + 1) / 2;
  Carver c(base);
  l.tab = c.take<double>(2 * BA_TAB);
  l.st = c.take<BaState>(1);
  l.cnt = c.take<int>(BA_COUNTERS);
  l.dc = c.take<double>(192);
  l.X = c.take<double>(2 * N * 3);
  l.set = c.take<uint32_t>(N);
  l.lm = c.take<uint8_t>(N);
  l.moves = c.take<uint8_t>(N);
  l.pt = c.take<double>(N * 9);
  l.cparts = c.take<double>((N + BA_THREADS - 1) / BA_THREADS);
  l.parts = c.take<double>(pairs * chunks * BA_SUMS);
  l.bytes = c.bytes;
  return l;
}

// ---- one observation ------------------------------------------------------------------------------------------------------
// The residual of X in the view and its exact Jacobians: rows (u, v) of Jc = d(du, dv) / d(w, dt) (6) and of Jp = d(du, dv) / dX
// (3).  With Y = R X + t: d/dY of du is ju = (fx a + s b), of dv is jv = fy b, a = (e0 - xn e2) / z, b = (e1 - yn e2) / z;
// dY/dX = R (Jp as in tv_normal), dY/dw = -[R X]x, dY/ddt = I.
struct BaObs {
  double du, dv;
  double cu[6], cv[6], pu[3], pv[3];
};

__device__ __forceinline__ BaObs ba_observe(const double* w, const TvPixel& q, const double* X) {
  const TvProj r = tv_project(w, q, X);
  const double* R = w + TV_R;
  BaObs o;
  o.du = r.du, o.dv = r.dv;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double a = (R[k] - r.xn * R[6 + k]) / r.z, b = (R[3 + k] - r.yn * R[6 + k]) / r.z;
    o.pu[k] = w[0] * a + w[4] * b;
    o.pv[k] = w[1] * b;
  }
  const double q0 = (R[0] * X[0] + R[1] * X[1]) + R[2] * X[2], q1 = (R[3] * X[0] + R[4] * X[1]) + R[5] * X[2],
               q2 = (R[6] * X[0] + R[7] * X[1]) + R[8] * X[2];
  const double a0 = 1.0 / r.z, a2 = (-r.xn) / r.z, b2 = (-r.yn) / r.z;
  const double u0 = w[0] * a0, u1 = w[4] * a0, u2 = w[0] * a2 + w[4] * b2;
  const double v1 = w[1] * a0, v2 = w[1] * b2;
  o.cu[0] = u2 * q1 - u1 * q2, o.cu[1] = u0 * q2 - u2 * q0, o.cu[2] = u1 * q0 - u0 * q1;
  o.cu[3] = u0, o.cu[4] = u1, o.cu[5] = u2;
  o.cv[0] = v2 * q1 - v1 * q2, o.cv[1] = -(v2 * q0), o.cv[2] = v1 * q0;
  o.cv[3] = 0.0, o.cv[4] = v1, o.cv[5] = v2;
  return o;
}

// W = Jc^T Jp (6 x 3)
__device__ __forceinline__ void ba_w(const BaObs& o, double (&W)[6][3]) {
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int k = 0; k < 3; ++k) W[i][k] = o.cu[i] * o.pu[k] + o.cv[i] * o.pv[k];
}

__device__ __forceinline__ void ba_load_tab(double* dst, const double* __restrict__ src, int V) {
  for (int i = threadIdx.x; i < V * TV_ROW; i += blockDim.x) dst[i] = src[i];
}

// a sum per wavefront by the fixed butterfly (each lane ends with the same bits)
__device__ __forceinline__ double ba_wave_sum(double a) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a = a + __shfl_xor(a, off);
  return a;
}

__device__ __forceinline__ int ba_wave_sum(int a) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a = a + __shfl_xor(a, off);
  return a;
}

// ---- kernels --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BA_THREADS) void ba_init_kernel(const int32_t* __restrict__ found, double lambda0, BaState* __restrict__ st,
                                                             int* __restrict__ cnt) {
  for (int i = threadIdx.x; i < BA_COUNTERS; i += BA_THREADS) cnt[i] = 0;
  if (threadIdx.x < TV_MAX_VIEWS) st->slot[threadIdx.x] = -1;
  if (threadIdx.x != 0) return;
  st->lambda = lambda0, st->cost = 0.0, st->cost_first = 0.0;
  st->cur = 0, st->done = 0, st->bad = 0, st->found = found ? (found[0] != 0) : 1;
  st->F = 0, st->nobs = 0, st->nfrozen = 0, st->nlandmarks = 0, st->kept = 0, st->rejected = 0, st->rounds_run = 0;
  st->free_mask = 0;
}

// the eligible observations of the round at the current state, before the starved views leave; round 0 copies X_in
__global__ __launch_bounds__(BA_THREADS) void ba_count_kernel(const double* __restrict__ points, const uint8_t* __restrict__ visible,
                                                              const double* __restrict__ X_in, int V, int n, int round, float thr, double dist,
                                                              const BaState* __restrict__ st, const double* __restrict__ tabs,
                                                              double* __restrict__ Xs, uint32_t* __restrict__ set, int* __restrict__ cnt) {
  __shared__ double tab[BA_TAB];
  if (!st->found) return;   // uniform
  const int cur = st->cur;
  ba_load_tab(tab, tabs + cur * BA_TAB, V);
  __syncthreads();
  const size_t N = (size_t)n;
  const size_t p = (size_t)blockIdx.x * BA_THREADS + threadIdx.x;
  const bool in = p < N;
  uint32_t bits = 0;
  if (in) {
    double X[3];
    const double* src = round == 0 ? X_in + p * 3 : Xs + ((size_t)cur * N + p) * 3;
#pragma unroll
    for (int i = 0; i < 3; ++i) X[i] = src[i];
    if (round == 0) {
#pragma unroll
      for (int i = 0; i < 3; ++i) Xs[p * 3 + i] = X[i];
    }
    const bool Xok = isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]);
    for (int v = 0; v < V; ++v) {
      const bool vis = visible ? visible[(size_t)v * N + p] != 0 : true;
      if (!(vis && Xok && tab[v * TV_ROW + TV_OK] != 0.0)) continue;
      const TvPixel q = tv_pixel(points, N, v, p);
      if (!q.finite) continue;
      const TvProj r = tv_project(tab + v * TV_ROW, q, X);
      const bool take = round == 0 ? r.z > 0.0 : (r.z > 0.0 && r.z < dist && (float)r.e <= thr);
      if (take) bits |= 1u << v;
    }
    set[p] = bits;
  }
  for (int v = 0; v < V; ++v) {
    const int c = __popcll(__ballot((bits >> v & 1u) != 0));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(cnt + round * TV_MAX_VIEWS + v, c);
  }
}

// the cost of a workgroup's 256 points (a thread a point) -> cparts: every wavefront by the butterfly, the wavefronts in order
__device__ __forceinline__ void ba_chunk_cost(double e, double* sh, double* __restrict__ cparts) {
  e = ba_wave_sum(e);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = e;
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = sh[0];
    for (int w = 1; w < BA_THREADS / 64; ++w) a = a + sh[w];
    cparts[blockIdx.x] = a;
  }
}

__global__ __launch_bounds__(BA_THREADS) void ba_classify_kernel(const double* __restrict__ points, int V, int n, int round, uint32_t fixed,
                                                                 const BaState* __restrict__ st, const double* __restrict__ tabs,
                                                                 const double* __restrict__ Xs, uint32_t* __restrict__ set,
                                                                 uint8_t* __restrict__ lm, uint8_t* __restrict__ used, int* __restrict__ cnt,
                                                                 double* __restrict__ cparts) {
  __shared__ double tab[BA_TAB];
  __shared__ double sh[BA_THREADS / 64];
  if (!st->found) return;   // uniform
  const int cur = st->cur;
  ba_load_tab(tab, tabs + cur * BA_TAB, V);
  __syncthreads();
  uint32_t frozen = 0;
  for (int v = 0; v < V; ++v)
    if (!(fixed >> v & 1u) && cnt[round * TV_MAX_VIEWS + v] < BA_MIN_VIEW_OBS) frozen |= 1u << v;
  const size_t N = (size_t)n;
  const size_t p = (size_t)blockIdx.x * BA_THREADS + threadIdx.x;
  double e = 0.0;
  int obs = 0, lms = 0;
  if (p < N) {
    const uint32_t bits = set[p] & ~frozen;
    const bool landmark = __popc(bits) < 2;
    set[p] = bits;
    lm[p] = landmark ? 1 : 0;
    obs += __popc(bits);
    lms += landmark ? 1 : 0;
    const double* Xp = Xs + ((size_t)cur * N + p) * 3;
    const double X[3] = {Xp[0], Xp[1], Xp[2]};
    for (int v = 0; v < V; ++v) {
      const bool u = (bits >> v & 1u) != 0;
      used[(size_t)v * N + p] = u ? 1 : 0;
      if (u) e += tv_project(tab + v * TV_ROW, tv_pixel(points, N, v, p), X).e;
    }
  }
  obs = ba_wave_sum(obs), lms = ba_wave_sum(lms);
  if ((threadIdx.x & 63) == 0) {
    if (obs) atomicAdd(cnt + BA_CNT_OBS + round, obs);
    if (lms) atomicAdd(cnt + BA_CNT_LM + round, lms);
  }
  ba_chunk_cost(e, sh, cparts);
}

// the cost partials summed by one wavefront: lane l adds partials l, l + 64, ... in ascending order, then the butterfly
__device__ __forceinline__ double ba_cost_sum(const double* __restrict__ cparts, int parts) {
  double a = 0.0;
  for (int c = threadIdx.x; c < parts; c += 64) a = a + cparts[c];
  return ba_wave_sum(a);
}

__global__ __launch_bounds__(64) void ba_begin_kernel(int V, int parts, int round, uint32_t fixed, double lambda0, BaState* __restrict__ st,
                                                      const int* __restrict__ cnt, const double* __restrict__ cparts) {
  if (!st->found) return;   // uniform
  const double a = ba_cost_sum(cparts, parts);
  if (threadIdx.x != 0) return;
  st->cost = a;
  if (round == 0) st->cost_first = a;
  st->lambda = lambda0;
  int F = 0, frozen = 0;
  uint32_t mask = 0;
  for (int v = 0; v < V; ++v) {
    const bool is_fixed = (fixed >> v & 1u) != 0;
    const bool is_free = !is_fixed && cnt[round * TV_MAX_VIEWS + v] >= BA_MIN_VIEW_OBS;
    st->slot[v] = is_free ? F : -1;
    if (is_free) mask |= 1u << v, ++F;
    if (!is_fixed && !is_free) ++frozen;
  }
  st->free_mask = mask;
  st->F = F, st->nfrozen = frozen;
  st->nobs = cnt[BA_CNT_OBS + round], st->nlandmarks = cnt[BA_CNT_LM + round];
  st->rounds_run = st->rounds_run + 1;
  st->bad = 0;
  st->done = (F == 0 || st->nobs == 0) ? 1 : 0;
}

__global__ __launch_bounds__(BA_THREADS) void ba_points_kernel(const double* __restrict__ points, int V, int n, const BaState* __restrict__ st,
                                                               const double* __restrict__ tabs, const double* __restrict__ Xs,
                                                               const uint32_t* __restrict__ set, const uint8_t* __restrict__ lm,
                                                               uint8_t* __restrict__ moves, double* __restrict__ pt) {
  __shared__ double tab[BA_TAB];
  if (!st->found || st->done) return;   // uniform
  const int cur = st->cur;
  const double damp = 1.0 + st->lambda;
  ba_load_tab(tab, tabs + cur * BA_TAB, V);
  __syncthreads();
  const size_t N = (size_t)n;
  const size_t p = (size_t)blockIdx.x * BA_THREADS + threadIdx.x;
  if (p >= N) return;
  const uint32_t bits = set[p];
  const double* Xp = Xs + ((size_t)cur * N + p) * 3;
  const double X[3] = {Xp[0], Xp[1], Xp[2]};
  double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
  for (int v = 0; v < V; ++v) {
    if (!(bits >> v & 1u)) continue;
    const BaObs o = ba_observe(tab + v * TV_ROW, tv_pixel(points, N, v, p), X);
    A[0] += o.pu[0] * o.pu[0] + o.pv[0] * o.pv[0];
    A[1] += o.pu[0] * o.pu[1] + o.pv[0] * o.pv[1];
    A[2] += o.pu[0] * o.pu[2] + o.pv[0] * o.pv[2];
    A[3] += o.pu[1] * o.pu[1] + o.pv[1] * o.pv[1];
    A[4] += o.pu[1] * o.pu[2] + o.pv[1] * o.pv[2];
    A[5] += o.pu[2] * o.pu[2] + o.pv[2] * o.pv[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] += o.pu[k] * o.du + o.pv[k] * o.dv;
  }
  const double m[6] = {A[0] * damp, A[1], A[2], A[3] * damp, A[4], A[5] * damp};
  // the cofactor rule of tv_solve, the inverse kept; its verdict on h is not asked: a step that is not finite fails the cost test
  double c[6], h[3];
  const double det = tv_cofactors(m, c);
  tv_solve(m, g, h);
  const bool go = !lm[p] && det != 0.0 && isfinite(det);
  double* o = pt + p * 9;
#pragma unroll
  for (int i = 0; i < 6; ++i) o[i] = go ? c[i] / det : 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) o[6 + i] = go ? h[i] : 0.0;
  moves[p] = go ? 1 : 0;
}

// pair index -> (v, w), v <= w: pairs are numbered w (w + 1) / 2 + v
__device__ __forceinline__ void ba_pair(int pair, int* v, int* w) {
  int b = 0;
  while ((b + 1) * (b + 2) / 2 <= pair) ++b;
  *w = b, *v = pair - b * (b + 1) / 2;
}

__global__ __launch_bounds__(BA_THREADS) void ba_pairs_kernel(const double* __restrict__ points, int V, int n, const BaState* __restrict__ st,
                                                              const double* __restrict__ tabs, const double* __restrict__ Xs,
                                                              const uint32_t* __restrict__ set, const uint8_t* __restrict__ moves,
                                                              const double* __restrict__ pt, double* __restrict__ parts) {
  __shared__ double rows[2 * TV_ROW];
  __shared__ double sh[BA_THREADS / 64][BA_SUMS];
  if (!st->found || st->done) return;   // uniform
  int v, w;
  ba_pair(blockIdx.x, &v, &w);
  const uint32_t free_mask = st->free_mask;
  if (!(free_mask >> v & 1u) || !(free_mask >> w & 1u)) return;   // uniform
  const int cur = st->cur;
  if (threadIdx.x < 2 * TV_ROW)
    rows[threadIdx.x] = tabs[cur * BA_TAB + (threadIdx.x < TV_ROW ? v * TV_ROW + threadIdx.x : w * TV_ROW + threadIdx.x - TV_ROW)];
  __syncthreads();
  const bool diag = v == w;
  const uint32_t need = 1u << v | 1u << w;
  double Y[6][6], U[21], b[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = 0; j < 6; ++j) Y[i][j] = 0.0;
    b[i] = 0.0;
  }
#pragma unroll
  for (int i = 0; i < 21; ++i) U[i] = 0.0;
  const size_t N = (size_t)n;
  const size_t base = (size_t)blockIdx.y * RS_CHUNK;
#pragma unroll 1
  for (int s = 0; s < RS_COUNT_STEPS; ++s) {   // every thread: its points in ascending order
    const size_t p = base + (size_t)s * BA_THREADS + threadIdx.x;
    if (p >= N) continue;
    if ((set[p] & need) != need) continue;
    const bool mv = moves[p] != 0;
    if (!diag && !mv) continue;
    const double* Xp = Xs + ((size_t)cur * N + p) * 3;
    const double X[3] = {Xp[0], Xp[1], Xp[2]};
    const BaObs ov = ba_observe(rows, tv_pixel(points, N, v, p), X);
    if (diag) {
      int k = 0;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) U[k] += ov.cu[i] * ov.cu[j] + ov.cv[i] * ov.cv[j], ++k;
        b[i] += ov.cu[i] * ov.du + ov.cv[i] * ov.dv;
      }
      if (!mv) continue;
    }
    double Wv[6][3], Ww[6][3], T[6][3];
    ba_w(ov, Wv);
    if (diag) {
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) Ww[i][k] = Wv[i][k];
    } else {
      ba_w(ba_observe(rows + TV_ROW, tv_pixel(points, N, w, p), X), Ww);
    }
    const double* q = pt + p * 9;
    const double i00 = q[0], i01 = q[1], i02 = q[2], i11 = q[3], i12 = q[4], i22 = q[5];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      T[i][0] = (Wv[i][0] * i00 + Wv[i][1] * i01) + Wv[i][2] * i02;
      T[i][1] = (Wv[i][0] * i01 + Wv[i][1] * i11) + Wv[i][2] * i12;
      T[i][2] = (Wv[i][0] * i02 + Wv[i][1] * i12) + Wv[i][2] * i22;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j) Y[i][j] += (T[i][0] * Ww[j][0] + T[i][1] * Ww[j][1]) + T[i][2] * Ww[j][2];
    if (diag) {
#pragma unroll
      for (int i = 0; i < 6; ++i) b[i] -= (Wv[i][0] * q[6] + Wv[i][1] * q[7]) + Wv[i][2] * q[8];
    }
  }
  // every wavefront: the fixed butterfly, then the 4 wavefronts in order
  const int wave = threadIdx.x >> 6;
  const bool lead = (threadIdx.x & 63) == 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const double a = ba_wave_sum(Y[i][j]);
      if (lead) sh[wave][i * 6 + j] = a;
    }
    const double a = ba_wave_sum(b[i]);
    if (lead) sh[wave][BA_B + i] = a;
  }
#pragma unroll
  for (int i = 0; i < 21; ++i) {
    const double a = ba_wave_sum(U[i]);
    if (lead) sh[wave][BA_U + i] = a;
  }
  __syncthreads();
  if ((int)threadIdx.x < BA_NSUMS) {
    double a = sh[0][threadIdx.x];
    for (int k = 1; k < BA_THREADS / 64; ++k) a = a + sh[k][threadIdx.x];
    parts[((size_t)blockIdx.x * gridDim.y + blockIdx.y) * BA_SUMS + threadIdx.x] = a;
  }
}

__global__ __launch_bounds__(BA_THREADS) void ba_solve_kernel(int V, int chunks, BaState* __restrict__ st, double* __restrict__ tabs,
                                                              const double* __restrict__ parts, double* __restrict__ dc) {
  // rows 0 .. m-1: S (lower triangle), row m: b; 187 * 188 / 2 doubles
  __shared__ double L[(BA_MAX_DIM + 1) * (BA_MAX_DIM + 2) / 2];
  __shared__ double xs[BA_MAX_DIM + 6];
  if (!st->found || st->done) return;   // uniform
  const int tid = threadIdx.x;
  const int cur = st->cur;
  const int m = 6 * st->F;
  const uint32_t free_mask = st->free_mask;
  const double damp = 1.0 + st->lambda;
  const int pairs = V * (V + 1) / 2;
  for (int e = tid; e < pairs * BA_SUMS; e += BA_THREADS) {
    const int pair = e >> 6, i = e & 63;
    int v, w;
    ba_pair(pair, &v, &w);
    if (!(free_mask >> v & 1u) || !(free_mask >> w & 1u)) continue;
    const int a = st->slot[v], b = st->slot[w];
    const double* src = parts + (size_t)pair * chunks * BA_SUMS;
    if (i < 36) {
      const int r = i / 6, c = i - r * 6;
      if (v == w && r < c) continue;
      double y = 0.0;
      for (int k = 0; k < chunks; ++k) y = y + src[(size_t)k * BA_SUMS + i];   // the chunks in chunk order
      if (v == w) {
        const int t = BA_U + c * 6 - c * (c - 1) / 2 + (r - c);
        double u = 0.0;
        for (int k = 0; k < chunks; ++k) u = u + src[(size_t)k * BA_SUMS + t];
        L[ch_tri(6 * a + r, 6 * a + c)] = (r == c ? u * damp : u) - y;
      } else {
        L[ch_tri(6 * b + c, 6 * a + r)] = -y;
      }
    } else if (v == w && i >= BA_B && i < BA_NSUMS) {
      double s = 0.0;
      for (int k = 0; k < chunks; ++k) s = s + src[(size_t)k * BA_SUMS + i];
      L[ch_tri(m, 6 * a + (i - BA_B))] = s;
    }
  }
  // Cholesky and both solves (chol.h); a pivot must be positive and finite
  const bool bad = !ch_factor<BA_THREADS>(L, m, [](int, double pivot) { return pivot > 0.0 && isfinite(pivot); });
  if (bad)
    for (int i = tid; i < m; i += BA_THREADS) xs[i] = 0.0;
  else
    ch_back<BA_THREADS>(L, m, xs);
  __syncthreads();
  for (int i = tid; i < m; i += BA_THREADS) dc[i] = xs[i];
  if (tid == 0) st->bad = bad ? 1 : 0;
  // the candidate poses: the current ones minus the step
  if (tid < V) {
    const double* src = tabs + cur * BA_TAB + tid * TV_ROW;
    double* dst = tabs + (1 - cur) * BA_TAB + tid * TV_ROW;
    for (int i = 0; i < TV_ROW; ++i) dst[i] = src[i];
    if (!bad && (free_mask >> tid & 1u)) {
      const double* d = xs + 6 * st->slot[tid];
      const double wv[3] = {-d[0], -d[1], -d[2]};
      double R[9], t[3];
      for (int i = 0; i < 9; ++i) R[i] = src[TV_R + i];
      rodrigues_rotate(wv, R);
      for (int i = 0; i < 3; ++i) t[i] = src[TV_T + i] - d[3 + i];
      for (int i = 0; i < 9; ++i) dst[TV_R + i] = R[i];
      for (int i = 0; i < 3; ++i) dst[TV_T + i] = t[i];
      for (int c = 0; c < 3; ++c) dst[TV_C + c] = -((R[c] * t[0] + R[3 + c] * t[1]) + R[6 + c] * t[2]);
    }
  }
}

__global__ __launch_bounds__(BA_THREADS) void ba_update_kernel(const double* __restrict__ points, int V, int n, const BaState* __restrict__ st,
                                                               const double* __restrict__ tabs, double* __restrict__ Xs,
                                                               const uint32_t* __restrict__ set, const uint8_t* __restrict__ moves,
                                                               const double* __restrict__ pt, const double* __restrict__ dc,
                                                               int* __restrict__ cnt, double* __restrict__ cparts) {
  __shared__ double tab[2 * BA_TAB];   // the current table, then the candidate's
  __shared__ double step[BA_MAX_DIM + 6];
  __shared__ int slot[TV_MAX_VIEWS];
  __shared__ double sh[BA_THREADS / 64];
  if (!st->found || st->done) return;   // uniform
  const int cur = st->cur;
  const uint32_t free_mask = st->free_mask;
  ba_load_tab(tab, tabs + cur * BA_TAB, V);
  ba_load_tab(tab + BA_TAB, tabs + (1 - cur) * BA_TAB, V);
  for (int i = threadIdx.x; i < 6 * st->F; i += BA_THREADS) step[i] = dc[i];
  if (threadIdx.x < TV_MAX_VIEWS) slot[threadIdx.x] = st->slot[threadIdx.x];
  __syncthreads();
  const size_t N = (size_t)n;
  const size_t p = (size_t)blockIdx.x * BA_THREADS + threadIdx.x;
  double e = 0.0;
  int behind = 0;
  if (p < N) {
    const uint32_t bits = set[p];
    const double* Xp = Xs + ((size_t)cur * N + p) * 3;
    double X[3] = {Xp[0], Xp[1], Xp[2]};
    if (moves[p]) {
      double a[3] = {0.0, 0.0, 0.0};
      for (int v = 0; v < V; ++v) {
        if (!(bits & free_mask & 1u << v)) continue;
        double W[6][3];
        ba_w(ba_observe(tab + v * TV_ROW, tv_pixel(points, N, v, p), X), W);
        const double* d = step + 6 * slot[v];
#pragma unroll
        for (int k = 0; k < 3; ++k)
          a[k] += ((((W[0][k] * d[0] + W[1][k] * d[1]) + W[2][k] * d[2]) + W[3][k] * d[3]) + W[4][k] * d[4]) + W[5][k] * d[5];
      }
      const double* q = pt + p * 9;
      X[0] = X[0] - (q[6] - ((q[0] * a[0] + q[1] * a[1]) + q[2] * a[2]));
      X[1] = X[1] - (q[7] - ((q[1] * a[0] + q[3] * a[1]) + q[4] * a[2]));
      X[2] = X[2] - (q[8] - ((q[2] * a[0] + q[4] * a[1]) + q[5] * a[2]));
    }
    double* Xc = Xs + ((size_t)(1 - cur) * N + p) * 3;
    Xc[0] = X[0], Xc[1] = X[1], Xc[2] = X[2];
    for (int v = 0; v < V; ++v) {
      if (!(bits >> v & 1u)) continue;
      const TvProj r = tv_project(tab + BA_TAB + v * TV_ROW, tv_pixel(points, N, v, p), X);
      e += r.e;
      behind += r.z > 0.0 ? 0 : 1;
    }
  }
  behind = ba_wave_sum(behind);
  if ((threadIdx.x & 63) == 0 && behind) atomicAdd(cnt + BA_CNT_BEHIND, behind);
  ba_chunk_cost(e, sh, cparts);
}

__global__ __launch_bounds__(64) void ba_decide_kernel(int parts, BaState* __restrict__ st, int* __restrict__ cnt,
                                                       const double* __restrict__ cparts) {
  if (!st->found || st->done) return;   // uniform
  const double a = ba_cost_sum(cparts, parts);
  if (threadIdx.x != 0) return;
  const int behind = cnt[BA_CNT_BEHIND];
  cnt[BA_CNT_BEHIND] = 0;
  if (!st->bad && behind == 0 && a < st->cost) {   // a NaN rejects
    st->cur = 1 - st->cur;
    st->cost = a;
    st->kept = st->kept + 1;
    const double l = st->lambda / 10.0;
    st->lambda = l > BA_LAMBDA_MIN ? l : BA_LAMBDA_MIN;
  } else {
    st->rejected = st->rejected + 1;
    st->lambda = 10.0 * st->lambda;
  }
  if (st->lambda > BA_LAMBDA_MAX) st->done = 1;
}

__global__ __launch_bounds__(BA_THREADS) void ba_finish_kernel(int V, int n, const BaState* __restrict__ st, const double* __restrict__ tabs,
                                                               const double* __restrict__ Xs, double* __restrict__ poses_out,
                                                               double* __restrict__ X_out, uint8_t* __restrict__ used, double* __restrict__ stats,
                                                               int32_t* __restrict__ info) {
  const bool found = st->found != 0;
  const int cur = st->cur;
  const size_t N = (size_t)n;
  const size_t p = (size_t)blockIdx.x * BA_THREADS + threadIdx.x;
  if (p < N) {
    const double* Xp = Xs + ((size_t)cur * N + p) * 3;
    for (int i = 0; i < 3; ++i) X_out[p * 3 + i] = found ? Xp[i] : 0.0;
    if (!found)
      for (int v = 0; v < V; ++v) used[(size_t)v * N + p] = 0;
  }
  if (blockIdx.x != 0) return;
  for (int i = threadIdx.x; i < V * 12; i += BA_THREADS) {
    const int v = i / 12, k = i - v * 12, r = k >> 2, c = k & 3;
    const double* w = tabs + cur * BA_TAB + v * TV_ROW;
    poses_out[i] = found ? (c < 3 ? w[TV_R + r * 3 + c] : w[TV_T + r]) : 0.0;
  }
  if (threadIdx.x == 0) {
    stats[0] = found ? st->cost_first : 0.0, stats[1] = found ? st->cost : 0.0, stats[2] = found ? st->lambda : 0.0, stats[3] = 0.0;
    info[0] = found ? 1 : 0, info[1] = found ? st->nobs : 0, info[2] = found ? st->F : 0, info[3] = found ? st->nfrozen : 0;
    info[4] = found ? st->nlandmarks : 0, info[5] = found ? st->kept : 0, info[6] = found ? st->rejected : 0;
    info[7] = found ? st->rounds_run : 0;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
namespace {

const char* const BA_FN = "cotr_bundle_adjust";

const char* ba_check_shape(int V, int n) {
  if (V < 2 || V > TV_MAX_VIEWS) return "V must be in [2, 32]";
  if (n < 1 || n > BA_MAX_POINTS) return "n must be in [1, 2^20]";
  return nullptr;
}

}  // namespace

extern "C" {

// per point: two copies of X, the set, two flags, the 9 doubles of ba_points; per 256 points a cost; per 2048-point chunk, for each of the
// V (V + 1) / 2 view pairs, 64 sums (the Jacobians are recomputed where they are needed instead of being stored: O(n + chunks pairs))
int cotr_bundle_adjust_scratch_bytes(int V, int n, size_t* bytes) {
  if (!bytes) return arg_fail("cotr_bundle_adjust_scratch_bytes", "bytes is NULL");
  if (const char* msg = ba_check_shape(V, n)) return arg_fail(BA_FN, msg);
  *bytes = ba_layout(nullptr, V, n).bytes;
  return COTR_OK;
}

int cotr_bundle_adjust(const double* points, const uint8_t* visible, const double* cams, const double* poses_in, const double* X_in,
                       const uint8_t* fixed_views, int V, int n, const int32_t* found, double threshold, double distance_thresh, int rounds,
                       int iters, double lambda0, double* poses_out, double* X_out, uint8_t* used_out, double* stats_out, int32_t* info_out,
                       void* scratch, size_t scratch_bytes, cotr_stream stream) {
  if (const char* msg = ba_check_shape(V, n)) return arg_fail(BA_FN, msg);
  if (!(threshold > 0.0) || !(threshold < INFINITY)) return arg_fail(BA_FN, "threshold must be finite and > 0");
  const float thr = (float)(threshold * threshold);
  if (!(thr > 0.0f) || !(thr < INFINITY)) return arg_fail(BA_FN, "the squared threshold must be a finite float32 that is not 0");
  if (!(distance_thresh > 0.0) || !(distance_thresh < INFINITY)) return arg_fail(BA_FN, "distance_thresh must be finite and > 0");
  if (rounds < 1 || rounds > BA_MAX_ROUNDS) return arg_fail(BA_FN, "rounds must be in [1, 8]");
  if (iters < 0 || iters > BA_MAX_ITERS) return arg_fail(BA_FN, "iters must be in [0, 64]");
  if (!(lambda0 >= BA_LAMBDA_MIN) || !(lambda0 <= BA_LAMBDA_MAX)) return arg_fail(BA_FN, "lambda0 must be in [1e-12, 1e12]");
  uint32_t fixed = 1u;
  if (fixed_views) {
    fixed = 0;
    for (int v = 0; v < V; ++v)
      if (fixed_views[v]) fixed |= 1u << v;
  }
  const uint32_t all = V == 32 ? 0xffffffffu : (1u << V) - 1u;
  if (fixed == 0) return arg_fail(BA_FN, "at least one view must be fixed");
  if (fixed == all) return arg_fail(BA_FN, "at least one view must not be fixed");
  if (!points || !cams || !poses_in || !X_in || !poses_out || !X_out || !used_out || !stats_out || !info_out || !scratch)
    return arg_fail(BA_FN, "points, cams, poses_in, X_in, poses_out, X_out, used_out, stats_out, info_out and scratch must not be NULL");
  if (!aligned(points, 16) || !aligned(cams, 8) || !aligned(poses_in, 8) || !aligned(X_in, 8) || !aligned(poses_out, 8) || !aligned(X_out, 8) ||
      !aligned(stats_out, 8) || !aligned(info_out, 4) || !aligned(found, 4) || !aligned(scratch, 16))
    return arg_fail(BA_FN, "points and scratch must be 16-byte, other doubles 8-byte and ints 4-byte aligned");
  const BaScratch l = ba_layout(scratch, V, n);
  if (scratch_bytes < l.bytes) return arg_fail(BA_FN, "scratch is smaller than cotr_bundle_adjust_scratch_bytes");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int chunks = (n + RS_CHUNK - 1) / RS_CHUNK;
  const unsigned blocks = (unsigned)((n + BA_THREADS - 1) / BA_THREADS);
  const unsigned pairs = (unsigned)(V * (V + 1) / 2);
  hipLaunchKernelGGL(tv_prepare_kernel, dim3(1), dim3(64), 0, s, cams, poses_in, V, found, l.tab, info_out);
  hipLaunchKernelGGL(ba_init_kernel, dim3(1), dim3(BA_THREADS), 0, s, found, lambda0, l.st, l.cnt);
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(ba_count_kernel, dim3(blocks), dim3(BA_THREADS), 0, s, points, visible, X_in, V, n, r, thr, distance_thresh, l.st, l.tab,
                       l.X, l.set, l.cnt);
    hipLaunchKernelGGL(ba_classify_kernel, dim3(blocks), dim3(BA_THREADS), 0, s, points, V, n, r, fixed, l.st, l.tab, l.X, l.set, l.lm,
                       used_out, l.cnt, l.cparts);
    hipLaunchKernelGGL(ba_begin_kernel, dim3(1), dim3(64), 0, s, V, (int)blocks, r, fixed, lambda0, l.st, l.cnt, l.cparts);
    for (int it = 0; it < iters; ++it) {
      hipLaunchKernelGGL(ba_points_kernel, dim3(blocks), dim3(BA_THREADS), 0, s, points, V, n, l.st, l.tab, l.X, l.set, l.lm, l.moves, l.pt);
      hipLaunchKernelGGL(ba_pairs_kernel, dim3(pairs, (unsigned)chunks), dim3(BA_THREADS), 0, s, points, V, n, l.st, l.tab, l.X, l.set, l.moves,
                         l.pt, l.parts);
      hipLaunchKernelGGL(ba_solve_kernel, dim3(1), dim3(BA_THREADS), 0, s, V, chunks, l.st, l.tab, l.parts, l.dc);
      hipLaunchKernelGGL(ba_update_kernel, dim3(blocks), dim3(BA_THREADS), 0, s, points, V, n, l.st, l.tab, l.X, l.set, l.moves, l.pt,
                         l.dc, l.cnt, l.cparts);
      hipLaunchKernelGGL(ba_decide_kernel, dim3(1), dim3(64), 0, s, (int)blocks, l.st, l.cnt, l.cparts);
    }
  }
  hipLaunchKernelGGL(ba_finish_kernel, dim3(blocks), dim3(BA_THREADS), 0, s, V, n, l.st, l.tab, l.X, poses_out, X_out, used_out, stats_out,
                     info_out);
  return launched();
}

}  // extern "C"
