// The poses of N views from pairwise results: cotr_average_rotations (absolute rotations from relative ones over a graph of view
// pairs) and cotr_solve_positions (the camera centres and the points from the tracks with the rotations known), DESIGN.md 3h-19.
// Handle-less (handleless.h), stream-ordered, integer atomics only, every floating-point sum in a fixed order: the same input gives
// the same bits.  Compiled with -ffp-contract=off.  The camera rows, the pixel, its ray and the cofactor rule are those of
// structure.hip (view_table.h), the rotation step is rodrigues.h, the dense solves are chol.h.  Neither call takes a scratch: the
// rotations live in LDS, the position solve keeps its state in work_out, an output the header documents.
//
//   ar_kernel          one workgroup: the dead edges, the greedy tree, then iters robust Gauss-Newton steps on the graph, the outputs
//
//   sp_init_kernel     the view rows (R as given, no translation), the counters zeroed, the state
//   per round:
//     sp_count_kernel    a thread per point: the round's set before the starved views leave it, observations per view counted
//     sp_points_kernel   a thread per point: the starved views leave, A_p and its inverse by the cofactor rule, used_out
//     sp_pairs_kernel    (view pair v <= w) x (chunk): the sums of P_v A^-1 P_w, on the diagonal also of P_v, per chunk
//     sp_solve_kernel    one workgroup: the chunks in order, S in LDS, Cholesky of S + mu I, two runs of inverse iteration
//     sp_update_kernel   a thread per point: X_p at the raw centres, the depth signs counted, the cost per workgroup
//     sp_finish_kernel   sign and scale; X_out scaled, and by its first workgroup the centres, the poses, stats and info
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "chol.h"
#include "handleless.h"
#include "ransac.h"
#include "rodrigues.h"
#define TV_NO_PREPARE_KERNEL   // the view rows are built by sp_init_kernel: no poses, no table kernel
#include "view_table.h"

using namespace cotr_detail;

#define GP_THREADS 256
#define GP_MAX_DIM (3 * (TV_MAX_VIEWS - 1))   // 93 unknowns of either reduced system
#define GP_TRI ((GP_MAX_DIM + 1) * (GP_MAX_DIM + 2) / 2)

// ================================================================================================================================
// rotation averaging
// ================================================================================================================================
#define AR_MAX_EDGES (TV_MAX_VIEWS * (TV_MAX_VIEWS - 1))
#define AR_MAX_ITERS 64
#define AR_PIVOT_TOL 1e-9

// C = A B, C = A^T B (3 x 3, row-major)
__device__ __forceinline__ void gp_mul(const double* A, const double* B, double* C) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) C[i * 3 + j] = (A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j]) + A[i * 3 + 2] * B[6 + j];
}

__device__ __forceinline__ void gp_tmul(const double* A, const double* B, double* C) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) C[i * 3 + j] = (A[i] * B[j] + A[3 + i] * B[3 + j]) + A[6 + i] * B[6 + j];
}

// r = log(M): a = the vector of (M - M^T) / 2, s = |a|, c = (trace - 1) / 2, theta = atan2(s, c); r = a theta / s above s = 1e-8,
// r = a below it with c > 0, and near a half turn theta times the unit vector along the column of M + I with the largest diagonal
// entry (the first of equals).  Returns |r| as sqrt of the sum of its squares.
__device__ __forceinline__ double gp_log(const double* M, double* r) {
  const double a[3] = {(M[7] - M[5]) / 2.0, (M[2] - M[6]) / 2.0, (M[3] - M[1]) / 2.0};
  const double s = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
  const double c = (((M[0] + M[4]) + M[8]) - 1.0) / 2.0;
  const double th = atan2(s, c);
  if (s > 1e-8) {
    const double f = th / s;
    for (int i = 0; i < 3; ++i) r[i] = a[i] * f;
  } else if (c > 0.0) {
    for (int i = 0; i < 3; ++i) r[i] = a[i];
  } else {
    int k = 0;
    if (M[4] > M[k * 4]) k = 1;
    if (M[8] > M[k * 4]) k = 2;
    double b[3];
    for (int i = 0; i < 3; ++i) b[i] = M[i * 3 + k] + (i == k ? 1.0 : 0.0);
    const double len = sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
    for (int i = 0; i < 3; ++i) r[i] = th * (b[i] / len);
  }
  return sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
}

__global__ __launch_bounds__(GP_THREADS) void ar_kernel(const double* __restrict__ R_rel, const int32_t* __restrict__ edges,
                                                        const double* __restrict__ weights, const int32_t* __restrict__ found, int n, int E,
                                                        int root, int iters, double sigma0, double sigma_end, double edge_thresh,
                                                        double* __restrict__ R_out, double* __restrict__ edge_out,
                                                        int32_t* __restrict__ view_info, int32_t* __restrict__ info, double* __restrict__ stats) {
  __shared__ double L[GP_TRI];               // rows 0 .. m-1: the system (lower triangle), row m: the right-hand side
  __shared__ double xs[GP_MAX_DIM + 3], diag0[GP_MAX_DIM + 3];
  __shared__ double lap[TV_MAX_VIEWS * TV_MAX_VIEWS], rhs[TV_MAX_VIEWS * 3];
  __shared__ double Rs[TV_MAX_VIEWS * 9];
  __shared__ double wt[AR_MAX_EDGES], ew[AR_MAX_EDGES], nw[AR_MAX_EDGES], rn[AR_MAX_EDGES], er[AR_MAX_EDGES * 3];
  __shared__ int16_t ea[AR_MAX_EDGES], eb[AR_MAX_EDGES];
  __shared__ uint8_t live[AR_MAX_EDGES], part[AR_MAX_EDGES];
  __shared__ int lr[TV_MAX_VIEWS], slot[TV_MAX_VIEWS], view_of[TV_MAX_VIEWS];
  __shared__ int Fs;
  const int tid = threadIdx.x;

  // the dead edges
  for (int e = tid; e < E; e += GP_THREADS) {
    const int a = edges[2 * e], b = edges[2 * e + 1];
    const double w = weights ? weights[e] : 1.0;
    bool ok = a >= 0 && a < n && b >= 0 && b < n && a != b && (!found || found[e] != 0) && w > 0.0 && w < INFINITY;
    for (int i = 0; i < 9; ++i) ok = ok && fabs(R_rel[(size_t)e * 9 + i]) < INFINITY;
    live[e] = ok ? 1 : 0, part[e] = 0;
    ea[e] = (int16_t)(ok ? a : 0), eb[e] = (int16_t)(ok ? b : 0);
    wt[e] = ok ? w : 0.0, ew[e] = ok ? w : 0.0, rn[e] = NAN;
  }
  if (tid < TV_MAX_VIEWS) {
    lr[tid] = tid == root ? 0 : -1;
    for (int i = 0; i < 9; ++i) Rs[tid * 9 + i] = tid == root ? (i % 4 == 0 ? 1.0 : 0.0) : NAN;
  }
  __syncthreads();

  // the greedy tree: round k locates every view that a live edge joins to a view located before round k
  for (int k = 1; k < n; ++k) {
    int best = -1;
    if (tid < n && lr[tid] < 0) {
      double bw = 0.0;
      for (int e = 0; e < E; ++e) {
        if (!live[e]) continue;
        const int a = ea[e], b = eb[e];
        const int other = a == tid ? b : (b == tid ? a : -1);
        if (other < 0 || lr[other] < 0 || lr[other] >= k) continue;
        if (wt[e] > bw) bw = wt[e], best = e;
      }
    }
    double Rn[9];
    if (best >= 0) {
      double Re[9];
      for (int i = 0; i < 9; ++i) Re[i] = R_rel[(size_t)best * 9 + i];
      if (eb[best] == tid)
        gp_mul(Re, Rs + ea[best] * 9, Rn);    // R_j = R_ij R_i
      else
        gp_tmul(Re, Rs + eb[best] * 9, Rn);   // R_i = R_ij^T R_j
    }
    __syncthreads();
    if (best >= 0) {
      for (int i = 0; i < 9; ++i) Rs[tid * 9 + i] = Rn[i];
      lr[tid] = k;
    }
    __syncthreads();
  }
  if (tid == 0) {
    int F = 0;
    for (int v = 0; v < TV_MAX_VIEWS; ++v) {
      const bool is_free = v < n && v != root && lr[v] >= 0;
      slot[v] = is_free ? F : -1;
      if (is_free) view_of[F++] = v;
    }
    Fs = F;
  }
  __syncthreads();
  const int F = Fs, m = 3 * F;

  int steps = 0, reason = 0;
  for (int k = 0;; ++k) {
    // the residuals at the current rotations
    for (int e = tid; e < E; e += GP_THREADS) {
      const bool in = live[e] && lr[ea[e]] >= 0 && lr[eb[e]] >= 0;
      part[e] = in ? 1 : 0;
      if (!in) continue;
      double Re[9], T[9], M[9];
      for (int i = 0; i < 9; ++i) Re[i] = R_rel[(size_t)e * 9 + i];
      gp_mul(Re, Rs + ea[e] * 9, T);
      gp_tmul(Rs + eb[e] * 9, T, M);
      rn[e] = gp_log(M, er + e * 3);
    }
    __syncthreads();
    if (k == iters) break;
    if (F == 0) {
      reason = 1;
      break;
    }
    const double sg = ldexp(sigma0, -k);
    const double sigma = sg > sigma_end ? sg : sigma_end;
    for (int e = tid; e < E; e += GP_THREADS) {
      if (!part[e]) continue;
      const double q = rn[e] / sigma, d = 1.0 + q * q;
      nw[e] = wt[e] / (d * d);   // becomes w_e only when the step is taken
    }
    for (int i = tid; i < m * (m + 1) / 2 + m; i += GP_THREADS) L[i] = 0.0;
    __syncthreads();
    // per view, over its edges in ascending edge index
    if (tid < n) {
      const int v = tid;
      for (int u = 0; u < n; ++u) lap[v * TV_MAX_VIEWS + u] = 0.0;
      double d = 0.0, g[3] = {0.0, 0.0, 0.0};
      for (int e = 0; e < E; ++e) {
        if (!part[e]) continue;
        const int a = ea[e], b = eb[e];
        if (a != v && b != v) continue;
        const double w = nw[e];
        d = d + w;
        lap[v * TV_MAX_VIEWS + (a == v ? b : a)] -= w;
        for (int c = 0; c < 3; ++c) g[c] = a == v ? g[c] - w * er[e * 3 + c] : g[c] + w * er[e * 3 + c];
      }
      lap[v * TV_MAX_VIEWS + v] = d;
      for (int c = 0; c < 3; ++c) rhs[v * 3 + c] = g[c];
    }
    __syncthreads();
    for (int i = tid; i < F * F; i += GP_THREADS) {
      const int a = i / F, b = i - a * F;
      if (b > a) continue;
      const double val = lap[view_of[a] * TV_MAX_VIEWS + view_of[b]];
      for (int c = 0; c < 3; ++c) L[ch_tri(3 * a + c, 3 * b + c)] = val;
      if (a == b)
        for (int c = 0; c < 3; ++c) diag0[3 * a + c] = val, L[ch_tri(m, 3 * a + c)] = rhs[view_of[a] * 3 + c];
    }
    // (ch_factor begins with a barrier) a pivot must be positive, finite and above AR_PIVOT_TOL of its entry before the elimination
    const bool fail = !ch_factor<GP_THREADS>(L, m, [&](int col, double pivot) {
      return fabs(pivot) < INFINITY && pivot > 0.0 && pivot > AR_PIVOT_TOL * diag0[col];
    });
    if (fail) {
      reason = 2;
      break;
    }
    ch_back<GP_THREADS>(L, m, xs);
    for (int e = tid; e < E; e += GP_THREADS)
      if (part[e]) ew[e] = nw[e];
    if (tid < n && slot[tid] >= 0) {   // R_v <- R_v exp([x]x): the transpose turned by -x
      const double* x = xs + 3 * slot[tid];
      const double wv[3] = {-x[0], -x[1], -x[2]};
      double Rt[9];
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Rt[i * 3 + j] = Rs[tid * 9 + j * 3 + i];
      rodrigues_rotate(wv, Rt);
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Rs[tid * 9 + i * 3 + j] = Rt[j * 3 + i];
    }
    ++steps;
    __syncthreads();
  }

  // the outputs
  for (int i = tid; i < n * 9; i += GP_THREADS) R_out[i] = Rs[i];
  for (int e = tid; e < E; e += GP_THREADS) {
    const bool in = part[e] != 0;
    edge_out[(size_t)e * 4] = in ? rn[e] : NAN;
    edge_out[(size_t)e * 4 + 1] = in ? ew[e] : 0.0;
    edge_out[(size_t)e * 4 + 2] = live[e] ? 1.0 : 0.0;
    edge_out[(size_t)e * 4 + 3] = in && rn[e] <= edge_thresh ? 1.0 : 0.0;
  }
  if (tid < n) {
    int nl = 0, ni = 0;
    for (int e = 0; e < E; ++e) {
      if (!live[e] || (ea[e] != tid && eb[e] != tid)) continue;
      ++nl;
      if (part[e] && rn[e] <= edge_thresh) ++ni;
    }
    view_info[tid * 4] = lr[tid] >= 0 ? 1 : 0, view_info[tid * 4 + 1] = lr[tid], view_info[tid * 4 + 2] = nl, view_info[tid * 4 + 3] = ni;
  }
  if (tid == 0) {
    int nl = 0, ni = 0;
    double cost = 0.0, worst = 0.0;
    for (int e = 0; e < E; ++e) {
      if (live[e]) ++nl;
      if (!part[e]) continue;
      cost = cost + ew[e] * (rn[e] * rn[e]);
      if (rn[e] <= edge_thresh) {
        ++ni;
        if (rn[e] > worst) worst = rn[e];
      }
    }
    info[0] = F >= 1 && reason != 2 ? 1 : 0, info[1] = F + 1, info[2] = nl, info[3] = ni, info[4] = steps, info[5] = reason, info[6] = 0, info[7] = 0;
    stats[0] = cost, stats[1] = worst;
  }
}

// ================================================================================================================================
// positions
// ================================================================================================================================
#define SP_MAX_POINTS (1 << 20)
#define SP_MAX_ROUNDS 8
#define SP_MAX_POWER 64
#define SP_TAB (TV_MAX_VIEWS * TV_ROW)
// the sums of a view pair per chunk: Y = P_v A^-1 P_w (9, row-major) | U = P_v (6: 00 01 02 11 12 22) | unused
#define SP_SUMS 16
#define SP_U 9
#define SP_NSUMS 15

struct SpState {
  double mu, lam0, lam1, cost;
  int found, fail, F, rounds_run, dropped;
  int slot[TV_MAX_VIEWS];
};

// integer counters: observations per view and round | observations per round | points per round | positive and negative depths per round
#define SP_CNT_OBS (SP_MAX_ROUNDS * TV_MAX_VIEWS)
#define SP_CNT_PTS (SP_CNT_OBS + SP_MAX_ROUNDS)
#define SP_CNT_POS (SP_CNT_PTS + SP_MAX_ROUNDS)
#define SP_CNT_NEG (SP_CNT_POS + SP_MAX_ROUNDS)
#define SP_COUNTERS (SP_CNT_NEG + SP_MAX_ROUNDS)

// work_out, in doubles: the view rows | the state | the counters | the raw centres | A_p^-1 [n][6] | the cost per 256 points |
// the sums [pairs][chunks][16]
struct SpWork {
  double* tab;
  SpState* st;
  int* cnt;
  double* craw;
  double* ainv;
  double* cparts;
  double* parts;
  size_t doubles;
};

static SpWork sp_layout(double* base, int V, int n) {
  const size_t N = (size_t)n, chunks = (N + RS_CHUNK - 1) / RS_CHUNK, pairs = (size_t)V * (V + 1) / 2;
  static_assert(sizeof(SpState) <= 64 * sizeof(double), "the state has 64 doubles of work_out");
  size_t o = 0;
  auto take = [&](size_t count) {   // with a NULL base it only measures
    double* p = base ? base + o : nullptr;
    o += count;
    return p;
  };
  SpWork l;
  l.tab = take(SP_TAB);
  l.st = reinterpret_cast<SpState*>(take(64));
  l.cnt = reinterpret_cast<int*>(take((SP_COUNTERS + 1) / 2));
  l.craw = take(TV_MAX_VIEWS * 3);
  l.ainv = take(N * 6);
  l.cparts = take((N + GP_THREADS - 1) / GP_THREADS);
  l.parts = take(pairs * chunks * SP_SUMS);
  l.doubles = o;
  return l;
}

// the unit ray of the point's pixel in the view, in the world: R^T r / |r|
__device__ __forceinline__ void sp_ray(const double* w, const TvPixel& q, double* d) {
  double r[3];
  tv_view_ray(w, q.u, q.v, r);
  const double len = sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
  d[0] = r[0] / len, d[1] = r[1] / len, d[2] = r[2] / len;
}

// P = I - d d^T (00 01 02 11 12 22)
__device__ __forceinline__ void sp_proj(const double* d, double* P) {
  P[0] = 1.0 - d[0] * d[0], P[1] = -(d[0] * d[1]), P[2] = -(d[0] * d[2]);
  P[3] = 1.0 - d[1] * d[1], P[4] = -(d[1] * d[2]), P[5] = 1.0 - d[2] * d[2];
}

// y = P x of a symmetric P (00 01 02 11 12 22)
__device__ __forceinline__ void sp_symv(const double* P, const double* x, double* y) {
  y[0] = (P[0] * x[0] + P[1] * x[1]) + P[2] * x[2];
  y[1] = (P[1] * x[0] + P[3] * x[1]) + P[4] * x[2];
  y[2] = (P[2] * x[0] + P[4] * x[1]) + P[5] * x[2];
}

__device__ __forceinline__ void sp_load_tab(double* dst, const double* __restrict__ src, int V) {
  for (int i = threadIdx.x; i < V * TV_ROW; i += blockDim.x) dst[i] = src[i];
}

__device__ __forceinline__ double sp_wave_sum(double a) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a = a + __shfl_xor(a, off);
  return a;
}

__device__ __forceinline__ int sp_wave_sum(int a) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a = a + __shfl_xor(a, off);
  return a;
}

// the views placed in the round: valid, and the root or with at least min_obs observations counted
__device__ __forceinline__ uint32_t sp_placed(const double* tab, const int* __restrict__ cnt, int V, int round, int root, int min_obs) {
  uint32_t mask = 0;
  for (int v = 0; v < V; ++v)
    if (tab[v * TV_ROW + TV_OK] != 0.0 && (v == root || cnt[round * TV_MAX_VIEWS + v] >= min_obs)) mask |= 1u << v;
  return mask;
}

__global__ __launch_bounds__(64) void sp_init_kernel(const double* __restrict__ cams, const double* __restrict__ R,
                                                     const int32_t* __restrict__ located, const int32_t* __restrict__ found, int V, int root,
                                                     double* __restrict__ tab, SpState* __restrict__ st, int* __restrict__ cnt,
                                                     double* __restrict__ craw) {
  const int v = threadIdx.x;
  for (int i = v; i < SP_COUNTERS; i += 64) cnt[i] = 0;
  for (int i = v; i < TV_MAX_VIEWS * 3; i += 64) craw[i] = NAN;
  bool ok = false;
  if (v < V) {
    double* w = tab + v * TV_ROW;
    ok = !located || located[v] != 0;
    for (int i = 0; i < 5; ++i) {
      w[i] = cams[v * 5 + i];
      ok = ok && fabs(w[i]) < INFINITY;
    }
    ok = ok && w[0] != 0.0 && w[1] != 0.0;
    for (int i = 0; i < 9; ++i) {
      w[TV_R + i] = R[v * 9 + i];
      ok = ok && fabs(w[TV_R + i]) < INFINITY;
    }
    for (int i = TV_T; i < TV_ROW; ++i) w[i] = 0.0;
    w[TV_OK] = ok ? 1.0 : 0.0;
  }
  const unsigned long long valid = __ballot(ok);
  if (v < TV_MAX_VIEWS) st->slot[v] = -1;
  if (v != 0) return;
  st->mu = 0.0, st->lam0 = 0.0, st->lam1 = 0.0, st->cost = 0.0;
  st->found = (found ? found[0] != 0 : true) && (valid >> root & 1ull) ? 1 : 0;
  st->fail = 0, st->F = 0, st->rounds_run = 0, st->dropped = 0;
}

__global__ __launch_bounds__(GP_THREADS) void sp_count_kernel(const double* __restrict__ points, const uint8_t* __restrict__ visible, int V,
                                                              int n, int round, double threshold, const SpState* __restrict__ st,
                                                              const double* __restrict__ tabs, const double* __restrict__ C,
                                                              const double* __restrict__ X, uint8_t* __restrict__ used,
                                                              int* __restrict__ cnt) {
  __shared__ double tab[SP_TAB];
  __shared__ double Cs[TV_MAX_VIEWS * 3];
  if (!st->found || st->fail) return;   // uniform
  sp_load_tab(tab, tabs, V);
  if (round > 0)
    for (int i = threadIdx.x; i < V * 3; i += GP_THREADS) Cs[i] = C[i];
  __syncthreads();
  const size_t N = (size_t)n;
  const size_t p = (size_t)blockIdx.x * GP_THREADS + threadIdx.x;
  uint32_t bits = 0;
  if (p < N) {
    double Xp[3] = {0.0, 0.0, 0.0};
    if (round > 0)
      for (int i = 0; i < 3; ++i) Xp[i] = X[p * 3 + i];
    for (int v = 0; v < V; ++v) {
      const double* w = tab + v * TV_ROW;
      bool take = (visible ? visible[(size_t)v * N + p] != 0 : true) && w[TV_OK] != 0.0;
      if (take) {
        const TvPixel q = tv_pixel(points, N, v, p);
        take = q.finite;
        if (take && round > 0) {
          double d[3];
          sp_ray(w, q, d);
          const double e[3] = {Xp[0] - Cs[v * 3], Xp[1] - Cs[v * 3 + 1], Xp[2] - Cs[v * 3 + 2]};
          const double dep = (d[0] * e[0] + d[1] * e[1]) + d[2] * e[2];
          const double c0 = d[1] * e[2] - d[2] * e[1], c1 = d[2] * e[0] - d[0] * e[2], c2 = d[0] * e[1] - d[1] * e[0];
          const double ang = atan2(sqrt((c0 * c0 + c1 * c1) + c2 * c2), dep);
          take = dep > 0.0 && ang <= threshold / sqrt(fabs(w[0] * w[1]));   // a NaN drops the observation
        }
      }
      if (take) bits |= 1u << v;
      used[(size_t)v * N + p] = take ? 1 : 0;
    }
  }
  for (int v = 0; v < V; ++v) {
    const int c = __popcll(__ballot((bits >> v & 1u) != 0));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(cnt + round * TV_MAX_VIEWS + v, c);
  }
}

__global__ __launch_bounds__(GP_THREADS) void sp_points_kernel(const double* __restrict__ points, int V, int n, int round, int root, int min_obs,
                                                               const SpState* __restrict__ st, const double* __restrict__ tabs,
                                                               uint8_t* __restrict__ used, double* __restrict__ ainv, int* __restrict__ cnt) {
  __shared__ double tab[SP_TAB];
  if (!st->found || st->fail) return;   // uniform
  sp_load_tab(tab, tabs, V);
  __syncthreads();
  const uint32_t placed = sp_placed(tab, cnt, V, round, root, min_obs);
  const size_t N = (size_t)n;
  const size_t p = (size_t)blockIdx.x * GP_THREADS + threadIdx.x;
  int obs = 0, solved = 0;
  if (p < N) {
    uint32_t bits = 0;
    for (int v = 0; v < V; ++v)
      if (used[(size_t)v * N + p]) bits |= 1u << v;
    bits &= placed;
    double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, c[6];
    for (int v = 0; v < V; ++v) {   // the views ascending
      if (!(bits >> v & 1u)) continue;
      double d[3], P[6];
      sp_ray(tab + v * TV_ROW, tv_pixel(points, N, v, p), d);
      sp_proj(d, P);
      for (int i = 0; i < 6; ++i) A[i] += P[i];
    }
    const double det = tv_cofactors(A, c);
    const bool go = __popc(bits) >= 2 && det != 0.0 && isfinite(det);
    if (!go) bits = 0;
    for (int i = 0; i < 6; ++i) ainv[p * 6 + i] = go ? c[i] / det : 0.0;
    for (int v = 0; v < V; ++v) used[(size_t)v * N + p] = bits >> v & 1u;
    obs = __popc(bits), solved = go ? 1 : 0;
  }
  obs = sp_wave_sum(obs), solved = sp_wave_sum(solved);
  if ((threadIdx.x & 63) == 0) {
    if (obs) atomicAdd(cnt + SP_CNT_OBS + round, obs);
    if (solved) atomicAdd(cnt + SP_CNT_PTS + round, solved);
  }
}

// pair index -> (v, w), v <= w: pairs are numbered w (w + 1) / 2 + v
__device__ __forceinline__ void sp_pair(int pair, int* v, int* w) {
  int b = 0;
  while ((b + 1) * (b + 2) / 2 <= pair) ++b;
  *w = b, *v = pair - b * (b + 1) / 2;
}

__global__ __launch_bounds__(GP_THREADS) void sp_pairs_kernel(const double* __restrict__ points, int V, int n, int round, int root, int min_obs,
                                                              const SpState* __restrict__ st, const double* __restrict__ tabs,
                                                              const uint8_t* __restrict__ used, const double* __restrict__ ainv,
                                                              const int* __restrict__ cnt, double* __restrict__ parts) {
  __shared__ double tab[SP_TAB];
  __shared__ double sh[GP_THREADS / 64][SP_SUMS];
  if (!st->found || st->fail) return;   // uniform
  int v, w;
  sp_pair(blockIdx.x, &v, &w);
  sp_load_tab(tab, tabs, V);
  __syncthreads();
  const uint32_t placed = sp_placed(tab, cnt, V, round, root, min_obs);
  if (!(placed >> v & 1u) || !(placed >> w & 1u) || v == root || w == root) return;   // uniform
  const bool diag = v == w;
  double Y[9], U[6];
#pragma unroll
  for (int i = 0; i < 9; ++i) Y[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) U[i] = 0.0;
  const size_t N = (size_t)n;
  const size_t base = (size_t)blockIdx.y * RS_CHUNK;
#pragma unroll 1
  for (int s = 0; s < RS_COUNT_STEPS; ++s) {   // every thread: its points in ascending order
    const size_t p = base + (size_t)s * GP_THREADS + threadIdx.x;
    if (p >= N) continue;
    if (!used[(size_t)v * N + p] || !used[(size_t)w * N + p]) continue;
    double d[3], Pv[6], Pw[6];
    sp_ray(tab + v * TV_ROW, tv_pixel(points, N, v, p), d);
    sp_proj(d, Pv);
    if (diag) {
#pragma unroll
      for (int i = 0; i < 6; ++i) U[i] += Pv[i], Pw[i] = Pv[i];
    } else {
      sp_ray(tab + w * TV_ROW, tv_pixel(points, N, w, p), d);
      sp_proj(d, Pw);
    }
    const double* a = ainv + p * 6;
    const double Ai[6] = {a[0], a[1], a[2], a[3], a[4], a[5]};
    // T = P_v A^-1 (row i: the symmetric A^-1 applied to row i of P_v), Y += T P_w
    const double rows[3][3] = {{Pv[0], Pv[1], Pv[2]}, {Pv[1], Pv[3], Pv[4]}, {Pv[2], Pv[4], Pv[5]}};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double T[3], yr[3];
      sp_symv(Ai, rows[i], T);
      sp_symv(Pw, T, yr);
#pragma unroll
      for (int j = 0; j < 3; ++j) Y[i * 3 + j] += yr[j];
    }
  }
  // every wavefront: the fixed butterfly, then the 4 wavefronts in order
  const int wave = threadIdx.x >> 6;
  const bool lead = (threadIdx.x & 63) == 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const double a = sp_wave_sum(Y[i]);
    if (lead) sh[wave][i] = a;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double a = sp_wave_sum(U[i]);
    if (lead) sh[wave][SP_U + i] = a;
  }
  __syncthreads();
  if ((int)threadIdx.x < SP_NSUMS) {
    double a = sh[0][threadIdx.x];
    for (int k = 1; k < GP_THREADS / 64; ++k) a = a + sh[k][threadIdx.x];
    parts[((size_t)blockIdx.x * gridDim.y + blockIdx.y) * SP_SUMS + threadIdx.x] = a;
  }
}

// (a . b) of m entries by thread 0 in ascending order, the same value for every thread; two barriers
__device__ __forceinline__ double sp_dot(const double* a, const double* b, int m, double* cell) {
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < m; ++i) s = s + a[i] * b[i];
    *cell = s;
  }
  __syncthreads();
  const double s = *cell;
  __syncthreads();
  return s;
}

// the fixed start vectors of the two runs of inverse iteration
__device__ __forceinline__ double sp_start(int run, int i) {
  return run == 0 ? 1.0 + 0.5 * (double)(i % 3) + 0.125 * (double)(i / 3) : 1.0 + 0.25 * (double)((i * 5) % 7) - 0.0625 * (double)(i / 3);
}

__global__ __launch_bounds__(GP_THREADS) void sp_solve_kernel(int V, int chunks, int round, int root, int min_obs, int power_iters,
                                                              SpState* __restrict__ st, const double* __restrict__ tabs,
                                                              const int* __restrict__ cnt, const double* __restrict__ parts,
                                                              double* __restrict__ craw) {
  __shared__ double L[GP_TRI];   // rows 0 .. m-1: S + mu I (lower triangle), row m: the right-hand side
  __shared__ double xs[GP_MAX_DIM + 3], xv[GP_MAX_DIM + 3], v0[GP_MAX_DIM + 3];
  __shared__ double tab[SP_TAB];
  __shared__ int slot[TV_MAX_VIEWS];
  __shared__ int Fs, dropped;
  __shared__ double mus, cell;
  if (!st->found || st->fail) return;   // uniform
  const int tid = threadIdx.x;
  sp_load_tab(tab, tabs, V);
  __syncthreads();
  const uint32_t placed = sp_placed(tab, cnt, V, round, root, min_obs);
  if (tid == 0) {
    int F = 0, nd = 0;
    for (int v = 0; v < TV_MAX_VIEWS; ++v) {
      const bool is_free = v < V && v != root && (placed >> v & 1u);
      slot[v] = is_free ? F++ : -1;
      if (v < V && tab[v * TV_ROW + TV_OK] != 0.0 && !(placed >> v & 1u)) ++nd;
    }
    Fs = F, dropped = nd;
  }
  __syncthreads();
  const int F = Fs, m = 3 * F;
  if (tid < TV_MAX_VIEWS) st->slot[tid] = slot[tid];
  if (tid == 0) st->F = F, st->dropped = dropped, st->rounds_run = round + 1;
  if (F == 0) {   // uniform
    if (tid == 0) st->fail = 1;
    return;
  }
  const int pairs = V * (V + 1) / 2;
  for (int e = tid; e < pairs * SP_SUMS; e += GP_THREADS) {
    const int pair = e >> 4, i = e & 15;
    if (i >= 9) continue;
    int v, w;
    sp_pair(pair, &v, &w);
    const int a = slot[v], b = slot[w];
    if (a < 0 || b < 0) continue;
    const int r = i / 3, c = i - r * 3;
    if (v == w && r < c) continue;
    const double* src = parts + (size_t)pair * chunks * SP_SUMS;
    double y = 0.0;
    for (int k = 0; k < chunks; ++k) y = y + src[(size_t)k * SP_SUMS + i];   // the chunks in chunk order
    if (v == w) {
      const int t = SP_U + (c == 0 ? r : (c == 1 ? 2 + r : 5));   // (r, c), r >= c, of 00 01 02 11 12 22
      double u = 0.0;
      for (int k = 0; k < chunks; ++k) u = u + src[(size_t)k * SP_SUMS + t];
      L[ch_tri(3 * a + r, 3 * a + c)] = u - y;
    } else {
      L[ch_tri(3 * b + c, 3 * a + r)] = -y;
    }
  }
  __syncthreads();
  if (tid == 0) {
    double big = 0.0;
    for (int i = 0; i < m; ++i) big = L[ch_tri(i, i)] > big ? L[ch_tri(i, i)] : big;
    mus = 1e-12 * big;
  }
  __syncthreads();
  const double mu = mus;
  for (int i = tid; i < m; i += GP_THREADS) L[ch_tri(i, i)] += mu, xv[i] = sp_start(0, i);
  __syncthreads();
  double nrm = sqrt(sp_dot(xv, xv, m, &cell));
  for (int i = tid; i < m; i += GP_THREADS) xv[i] = xv[i] / nrm, L[ch_tri(m, i)] = xv[i];
  // (ch_factor begins with a barrier) a pivot must be positive and finite
  const bool bad = !ch_factor<GP_THREADS>(L, m, [](int, double pivot) { return pivot > 0.0 && isfinite(pivot); });
  if (bad) {   // uniform
    if (tid == 0) st->fail = 1;
    return;
  }
  double lam[2] = {0.0, 0.0};
  for (int run = 0; run < 2; ++run) {
    if (run == 1) {   // the second run: the start deflated by the first run's vector, as every iterate after it
      for (int i = tid; i < m; i += GP_THREADS) v0[i] = xv[i], xs[i] = sp_start(1, i);
      __syncthreads();
      const double a = sp_dot(xs, v0, m, &cell);
      for (int i = tid; i < m; i += GP_THREADS) xs[i] = xs[i] - a * v0[i];
      __syncthreads();
      nrm = sqrt(sp_dot(xs, xs, m, &cell));
      for (int i = tid; i < m; i += GP_THREADS) xv[i] = xs[i] / nrm;
      __syncthreads();
    }
    for (int it = 0; it < power_iters; ++it) {
      if (run == 1 || it > 0) {
        for (int i = tid; i < m; i += GP_THREADS) L[ch_tri(m, i)] = xv[i];
        ch_forward<GP_THREADS>(L, m);
      }
      ch_back<GP_THREADS>(L, m, xs);
      if (run == 1) {
        const double a = sp_dot(xs, v0, m, &cell);
        for (int i = tid; i < m; i += GP_THREADS) xs[i] = xs[i] - a * v0[i];
        __syncthreads();
      }
      lam[run] = 1.0 / sp_dot(xv, xs, m, &cell) - mu;
      nrm = sqrt(sp_dot(xs, xs, m, &cell));
      for (int i = tid; i < m; i += GP_THREADS) xv[i] = xs[i] / nrm;
      __syncthreads();
    }
  }
  // the raw centres: the first run's vector, the root at the origin
  if (tid < V * 3) {
    const int v = tid / 3, c = tid - v * 3;
    craw[tid] = slot[v] >= 0 ? v0[3 * slot[v] + c] : (v == root ? 0.0 : NAN);
  }
  if (tid == 0) st->mu = mu, st->lam0 = lam[0], st->lam1 = lam[1];
}

__global__ __launch_bounds__(GP_THREADS) void sp_update_kernel(const double* __restrict__ points, int V, int n, int round,
                                                               const SpState* __restrict__ st, const double* __restrict__ tabs,
                                                               const uint8_t* __restrict__ used, const double* __restrict__ ainv,
                                                               const double* __restrict__ craw, double* __restrict__ X, int* __restrict__ cnt,
                                                               double* __restrict__ cparts) {
  __shared__ double tab[SP_TAB];
  __shared__ double Cs[TV_MAX_VIEWS * 3];
  __shared__ double sh[GP_THREADS / 64];
  if (!st->found || st->fail) return;   // uniform
  sp_load_tab(tab, tabs, V);
  for (int i = threadIdx.x; i < V * 3; i += GP_THREADS) Cs[i] = craw[i];
  __syncthreads();
  const size_t N = (size_t)n;
  const size_t p = (size_t)blockIdx.x * GP_THREADS + threadIdx.x;
  double cost = 0.0;
  int pos = 0, neg = 0;
  if (p < N) {
    uint32_t bits = 0;
    for (int v = 0; v < V; ++v)
      if (used[(size_t)v * N + p]) bits |= 1u << v;
    double b[3] = {0.0, 0.0, 0.0}, Xp[3] = {NAN, NAN, NAN};
    if (bits) {
      for (int v = 0; v < V; ++v) {   // the views ascending
        if (!(bits >> v & 1u)) continue;
        double d[3], P[6], y[3];
        sp_ray(tab + v * TV_ROW, tv_pixel(points, N, v, p), d);
        sp_proj(d, P);
        sp_symv(P, Cs + v * 3, y);
        for (int i = 0; i < 3; ++i) b[i] += y[i];
      }
      sp_symv(ainv + p * 6, b, Xp);
      for (int v = 0; v < V; ++v) {
        if (!(bits >> v & 1u)) continue;
        double d[3];
        sp_ray(tab + v * TV_ROW, tv_pixel(points, N, v, p), d);
        const double e[3] = {Xp[0] - Cs[v * 3], Xp[1] - Cs[v * 3 + 1], Xp[2] - Cs[v * 3 + 2]};
        const double dep = (d[0] * e[0] + d[1] * e[1]) + d[2] * e[2];
        const double q[3] = {e[0] - d[0] * dep, e[1] - d[1] * dep, e[2] - d[2] * dep};
        cost += (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2];
        pos += dep > 0.0 ? 1 : 0, neg += dep < 0.0 ? 1 : 0;
      }
    }
    for (int i = 0; i < 3; ++i) X[p * 3 + i] = Xp[i];
  }
  pos = sp_wave_sum(pos), neg = sp_wave_sum(neg);
  if ((threadIdx.x & 63) == 0) {
    if (pos) atomicAdd(cnt + SP_CNT_POS + round, pos);
    if (neg) atomicAdd(cnt + SP_CNT_NEG + round, neg);
  }
  cost = sp_wave_sum(cost);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = cost;
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = sh[0];
    for (int w = 1; w < GP_THREADS / 64; ++w) a = a + sh[w];
    cparts[blockIdx.x] = a;
  }
}

__global__ __launch_bounds__(GP_THREADS) void sp_finish_kernel(int V, int n, int round, int root, int parts, const SpState* __restrict__ st,
                                                               const double* __restrict__ tabs, const int* __restrict__ cnt,
                                                               const double* __restrict__ craw, const double* __restrict__ cparts,
                                                               double* __restrict__ C_out, double* __restrict__ poses_out,
                                                               double* __restrict__ X, uint8_t* __restrict__ used, double* __restrict__ stats,
                                                               int32_t* __restrict__ info) {
  const bool found = st->found != 0, fail = st->fail != 0;
  if (found && st->rounds_run != round + 1) return;   // uniform: failed in an earlier round, whose outputs stand
  const size_t N = (size_t)n;
  const size_t p = (size_t)blockIdx.x * GP_THREADS + threadIdx.x;
  // sign and scale, by every thread alike: more negative depths than positive turn the solution round; the root-mean-square
  // distance of the other placed centres from the root becomes 1
  const int F = st->F;
  const int pos = cnt[SP_CNT_POS + round], neg = cnt[SP_CNT_NEG + round];
  const bool flip = neg > pos;
  double ss = 0.0;
  for (int v = 0; v < V; ++v)
    if (st->slot[v] >= 0) ss = ss + ((craw[v * 3] * craw[v * 3] + craw[v * 3 + 1] * craw[v * 3 + 1]) + craw[v * 3 + 2] * craw[v * 3 + 2]);
  const double s2 = (double)F / ss;
  const double s = flip ? -sqrt(s2) : sqrt(s2);
  if (p < N) {
    for (int i = 0; i < 3; ++i) X[p * 3 + i] = !found ? 0.0 : (fail ? NAN : X[p * 3 + i] * s);
    if (!found)
      for (int v = 0; v < V; ++v) used[(size_t)v * N + p] = 0;
  }
  if (blockIdx.x != 0) return;
  double cost = 0.0;
  if (found && !fail) {   // the cost partials by one wavefront: lane l adds partials l, l + 64, ... in ascending order, then the butterfly
    if (threadIdx.x < 64) {
      for (int c = threadIdx.x; c < parts; c += 64) cost = cost + cparts[c];
      cost = sp_wave_sum(cost);
    }
  }
  for (int i = threadIdx.x; i < V * 3; i += GP_THREADS) {
    const int v = i / 3;
    C_out[i] = !found ? 0.0 : (fail ? NAN : (v == root ? 0.0 : craw[i] * s));
  }
  for (int i = threadIdx.x; i < V * 12; i += GP_THREADS) {
    const int v = i / 12, k = i - v * 12, r = k >> 2, c = k & 3;
    const double* R = tabs + v * TV_ROW + TV_R;
    double val = 0.0;
    if (found) {
      if (c < 3) {
        val = R[r * 3 + c];
      } else if (fail) {
        val = NAN;
      } else if (v != root) {
        const double C[3] = {craw[v * 3] * s, craw[v * 3 + 1] * s, craw[v * 3 + 2] * s};
        val = -((R[r * 3] * C[0] + R[r * 3 + 1] * C[1]) + R[r * 3 + 2] * C[2]);
      }
    }
    poses_out[i] = val;
  }
  if (threadIdx.x == 0) {
    const bool ok = found && !fail;
    stats[0] = ok ? st->lam0 : 0.0, stats[1] = ok ? st->lam1 : 0.0, stats[2] = ok ? cost * s2 : 0.0, stats[3] = 0.0;
    info[0] = ok ? 1 : 0;
    info[1] = found ? cnt[SP_CNT_OBS + round] : 0;
    info[2] = ok ? F + 1 : 0;
    info[3] = found ? st->dropped : 0;
    info[4] = found ? cnt[SP_CNT_PTS + round] : 0;
    info[5] = ok ? (flip ? neg : pos) : 0;
    info[6] = ok ? (flip ? pos : neg) : 0;
    info[7] = found ? st->rounds_run : 0;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
namespace {

const char* const AR_FN = "cotr_average_rotations";
const char* const SP_FN = "cotr_solve_positions";

const char* sp_check_shape(int V, int n) {
  if (V < 2 || V > TV_MAX_VIEWS) return "V must be in [2, 32]";
  if (n < 1 || n > SP_MAX_POINTS) return "n must be in [1, 2^20]";
  return nullptr;
}

}  // namespace

extern "C" {

int cotr_average_rotations(const double* R_rel, const int32_t* edges, const double* weights, const int32_t* found, int n, int E, int root,
                           int iters, double sigma0, double sigma_end, double edge_thresh, double* R_out, double* edge_out,
                           int32_t* view_info_out, int32_t* info_out, double* stats_out, cotr_stream stream) {
  if (n < 2 || n > TV_MAX_VIEWS) return arg_fail(AR_FN, "n must be in [2, 32]");
  if (E < 1 || E > n * (n - 1)) return arg_fail(AR_FN, "E must be in [1, n (n - 1)]");
  if (root < 0 || root >= n) return arg_fail(AR_FN, "root must be in [0, n)");
  if (iters < 0 || iters > AR_MAX_ITERS) return arg_fail(AR_FN, "iters must be in [0, 64]");
  if (!(sigma_end > 0.0) || !(sigma0 >= sigma_end) || !(sigma0 < INFINITY)) return arg_fail(AR_FN, "0 < sigma_end <= sigma0 must be finite");
  if (!(edge_thresh > 0.0) || !(edge_thresh < INFINITY)) return arg_fail(AR_FN, "edge_thresh must be finite and > 0");
  if (!R_rel || !edges || !R_out || !edge_out || !view_info_out || !info_out || !stats_out)
    return arg_fail(AR_FN, "R_rel, edges, R_out, edge_out, view_info_out, info_out and stats_out must not be NULL");
  if (!aligned(R_rel, 8) || !aligned(weights, 8) || !aligned(R_out, 8) || !aligned(edge_out, 8) || !aligned(stats_out, 8) || !aligned(edges, 4) ||
      !aligned(found, 4) || !aligned(view_info_out, 4) || !aligned(info_out, 4))
    return arg_fail(AR_FN, "doubles must be 8-byte and ints 4-byte aligned");
  hipLaunchKernelGGL(ar_kernel, dim3(1), dim3(GP_THREADS), 0, static_cast<hipStream_t>(stream), R_rel, edges, weights, found, n, E, root, iters,
                     sigma0, sigma_end, edge_thresh, R_out, edge_out, view_info_out, info_out, stats_out);
  return launched();
}

int cotr_solve_positions_work_doubles(int V, int n, size_t* doubles) {
  if (!doubles) return arg_fail("cotr_solve_positions_work_doubles", "doubles is NULL");
  if (const char* msg = sp_check_shape(V, n)) return arg_fail(SP_FN, msg);
  *doubles = sp_layout(nullptr, V, n).doubles;
  return COTR_OK;
}

int cotr_solve_positions(const double* points, const uint8_t* visible, const double* cams, const double* R, const int32_t* located, int V,
                         int n, const int32_t* found, int root, double threshold, int rounds, int min_obs, int power_iters, double* C_out,
                         double* poses_out, double* X_out, uint8_t* used_out, double* stats_out, int32_t* info_out, double* work_out,
                         cotr_stream stream) {
  if (const char* msg = sp_check_shape(V, n)) return arg_fail(SP_FN, msg);
  if (root < 0 || root >= V) return arg_fail(SP_FN, "root must be in [0, V)");
  if (!(threshold > 0.0) || !(threshold < INFINITY)) return arg_fail(SP_FN, "threshold must be finite and > 0");
  if (rounds < 1 || rounds > SP_MAX_ROUNDS) return arg_fail(SP_FN, "rounds must be in [1, 8]");
  if (min_obs < 1) return arg_fail(SP_FN, "min_obs must be >= 1");
  if (power_iters < 1 || power_iters > SP_MAX_POWER) return arg_fail(SP_FN, "power_iters must be in [1, 64]");
  if (!points || !cams || !R || !C_out || !poses_out || !X_out || !used_out || !stats_out || !info_out || !work_out)
    return arg_fail(SP_FN, "points, cams, R, C_out, poses_out, X_out, used_out, stats_out, info_out and work_out must not be NULL");
  if (!aligned(points, 16) || !aligned(cams, 8) || !aligned(R, 8) || !aligned(C_out, 8) || !aligned(poses_out, 8) || !aligned(X_out, 8) ||
      !aligned(stats_out, 8) || !aligned(work_out, 8) || !aligned(info_out, 4) || !aligned(found, 4) || !aligned(located, 4))
    return arg_fail(SP_FN, "points must be 16-byte, other doubles 8-byte and ints 4-byte aligned");
  const SpWork l = sp_layout(work_out, V, n);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int chunks = (n + RS_CHUNK - 1) / RS_CHUNK;
  const unsigned blocks = (unsigned)((n + GP_THREADS - 1) / GP_THREADS);
  const unsigned pairs = (unsigned)(V * (V + 1) / 2);
  hipLaunchKernelGGL(sp_init_kernel, dim3(1), dim3(64), 0, s, cams, R, located, found, V, root, l.tab, l.st, l.cnt, l.craw);
  for (int r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(sp_count_kernel, dim3(blocks), dim3(GP_THREADS), 0, s, points, visible, V, n, r, threshold, l.st, l.tab,
                       (const double*)C_out, (const double*)X_out, used_out, l.cnt);
    hipLaunchKernelGGL(sp_points_kernel, dim3(blocks), dim3(GP_THREADS), 0, s, points, V, n, r, root, min_obs, l.st, l.tab, used_out, l.ainv,
                       l.cnt);
    hipLaunchKernelGGL(sp_pairs_kernel, dim3(pairs, (unsigned)chunks), dim3(GP_THREADS), 0, s, points, V, n, r, root, min_obs, l.st, l.tab,
                       (const uint8_t*)used_out, l.ainv, l.cnt, l.parts);
    hipLaunchKernelGGL(sp_solve_kernel, dim3(1), dim3(GP_THREADS), 0, s, V, chunks, r, root, min_obs, power_iters, l.st, l.tab, l.cnt, l.parts,
                       l.craw);
    hipLaunchKernelGGL(sp_update_kernel, dim3(blocks), dim3(GP_THREADS), 0, s, points, V, n, r, l.st, l.tab, (const uint8_t*)used_out, l.ainv,
                       l.craw, X_out, l.cnt, l.cparts);
    hipLaunchKernelGGL(sp_finish_kernel, dim3(blocks), dim3(GP_THREADS), 0, s, V, n, r, root, (int)blocks, l.st, l.tab, l.cnt, l.craw,
                       l.cparts, C_out, poses_out, X_out, used_out, stats_out, info_out);
  }
  return launched();
}

}  // extern "C"
