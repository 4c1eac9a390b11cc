// Joint refinement of the poses of n depth maps of one size: point-to-plane ICP over every ordered pair (edge) of a graph of
// views, one Gauss-Newton step on all free poses together (multi-way ICP).  Rules in DESIGN.md 3h-15.  Poses are
// camera-to-world; a step perturbs them by a world-frame twist about `centre`.
//
// cotr_icp_maps: 2 launches:
//   1. im_maps_begin_kernel     zeroes info_out
//   2. im_map_kernel            one thread per pixel of every capture: the pixel rule of icp_maps.h -> maps_out, interleaved
// cotr_icp_multiview: 1 + 2 * (iters + 1) launches on the caller's stream, whatever the data:
//   1. im_begin_kernel          one workgroup: c2w0 -> c2w_out (the working poses), the counters zeroed, the live edges counted
//   2. iters + 1 pairs of
//      im_edge_kernel           one workgroup per (edge, band of source rows): the gates and the residual of cotr_icp_depth at
//                               R_ab, t_ab of the working poses, 29 sums and the usable pixels: every thread over its pixels in
//                               order, every wavefront in a fixed butterfly, the 4 wavefronts in order -> edge_out[e][band]
//      im_solve_kernel          one workgroup: the bands of every edge in band order, the edge gate, the free views, the packed
//                               lower triangle of the 6F x 6F system with its right-hand side in LDS (every entry added up by one
//                               thread in a fixed order), Cholesky by columns and both solves (chol.h), the twist of every free view
//      The last pair only evaluates.  The stop reason in info_out idles the chain after a stop; its length never depends on the
//      data.
// All device state lives in the documented outputs (c2w_out, edge_out, info_out): there is no scratch.  Integer atomics only:
// the same input gives the same bits.  No host waits, no allocation: capturable.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "chol.h"
#include "handleless.h"
#include "icp_maps.h"
#include "ransac.h"
#include "refit.h"
#include "rodrigues.h"
#include "view_table.h"

using namespace cotr_detail;

#define IM_THREADS 256
#define IM_BANDS 8             // the source rows of an edge are cut into this many bands, one workgroup each
#define IM_ROW 32              // a row of edge_out: 29 sums, the usable source pixels, 0, 0
#define IM_SUMS 29             // 21 of J^T J, 6 of J^T r, the squared error, the pairs
#define IM_EDGE (IM_BANDS * IM_ROW)
#define IM_MIN_PAIRS 6
#define IM_MAX_ITERS 64
#define IM_MAX_STRIDE 64
#define IM_MAX_DIM (6 * (TV_MAX_VIEWS - 1))   // 186 unknowns: at least one view is fixed
#define IM_TAB (TV_MAX_VIEWS * TV_MAX_VIEWS)

struct ImGrid {
  int n, H, W, stride, ws, hs;   // ws, hs: source pixels in a row, source rows
  double max_d2, normal_cos;
  double c[3];                   // the centre of the twists
};

// ---- the maps -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void im_maps_begin_kernel(int n, int32_t* __restrict__ info) {
  for (int i = threadIdx.x; i < n * 4; i += 64) info[i] = 0;
}

// grid (pixels / 256, n): maps_out[c][H W][6] = vertex, normal (NaN where there is none); info[c] = {vertices, normals, 0, 0}
__global__ __launch_bounds__(256) void im_map_kernel(const float* __restrict__ depths, int H, int W, EsCams cams, double edge,
                                                     double* __restrict__ maps_out, int32_t* __restrict__ info) {
  const int c = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const size_t hw = (size_t)H * W;
  bool has_v = false, has_n = false;
  if (p < H * W) {
    const int y = p / W, x = p - y * W;
    double v[3], n[3];
    has_n = ic_pixel(depths + (size_t)c * hw, H, W, cams.k[c], edge, x, y, v, n);
    has_v = v[0] == v[0];
    double* o = maps_out + ((size_t)c * hw + p) * 6;
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = v[i], o[3 + i] = n[i];
  }
  const int cv = __popcll(__ballot(has_v)), cn = __popcll(__ballot(has_n));
  if ((threadIdx.x & 63) == 0) {
    if (cv > 0) atomicAdd(&info[c * 4], cv);
    if (cn > 0) atomicAdd(&info[c * 4 + 1], cn);
  }
}

// ---- the chain ------------------------------------------------------------------------------------------------------------
// whether (a, b) names two different views of the call that were both found
__device__ __forceinline__ bool im_edge_valid(int a, int b, int n, const int32_t* __restrict__ found) {
  if (a < 0 || a >= n || b < 0 || b >= n || a == b) return false;
  return !found || (found[a] != 0 && found[b] != 0);
}

__global__ __launch_bounds__(IM_THREADS) void im_begin_kernel(int n, int E, const double* c2w0, const int32_t* __restrict__ edges,
                                                               const int32_t* __restrict__ found, double* poses, int32_t* __restrict__ info,
                                                               int32_t* __restrict__ view_info, double* __restrict__ stats) {
  __shared__ int first[IM_TAB];   // the first edge that names an ordered pair
  __shared__ int live;
  const int tid = threadIdx.x;
  for (int i = tid; i < IM_TAB; i += IM_THREADS) first[i] = INT_MAX;
  if (tid == 0) live = 0;
  __syncthreads();
  for (int e = tid; e < E; e += IM_THREADS) {
    const int a = edges[2 * e], b = edges[2 * e + 1];
    if (im_edge_valid(a, b, n, found)) atomicMin(&first[a * TV_MAX_VIEWS + b], e);
  }
  __syncthreads();
  for (int e = tid; e < E; e += IM_THREADS) {
    const int a = edges[2 * e], b = edges[2 * e + 1];
    if (im_edge_valid(a, b, n, found) && first[a * TV_MAX_VIEWS + b] == e) atomicAdd(&live, 1);
  }
  __syncthreads();
  for (int i = tid; i < n * 16; i += IM_THREADS) poses[i] = c2w0[i];
  for (int i = tid; i < n * 4; i += IM_THREADS) view_info[i] = 0;
  if (tid < 2) stats[tid] = 0.0;
  if (tid < 8) info[tid] = tid == 4 ? live : 0;
}

// grid (IM_BANDS, E).  Edge e = (a, b): A = view a is the target, B = view b the source.
__global__ __launch_bounds__(IM_THREADS) void im_edge_kernel(const double* __restrict__ maps, EsCams cams, ImGrid g, const int32_t* __restrict__ edges,
                                                              const int32_t* __restrict__ found, const double* __restrict__ poses,
                                                              const int32_t* __restrict__ info, double* __restrict__ edge_out,
                                                              int32_t* __restrict__ assoc) {
  __shared__ double sh[IM_THREADS / 64][IM_ROW];
  if (info[3] != 0) return;   // stopped: uniform
  const int s = blockIdx.x, e = blockIdx.y, tid = threadIdx.x;
  const int a = edges[2 * e], b = edges[2 * e + 1];
  const bool valid = im_edge_valid(a, b, g.n, found);
  int dup = 0;
  if (valid)
    for (int j = tid; j < e; j += IM_THREADS) dup |= (edges[2 * j] == a && edges[2 * j + 1] == b) ? 1 : 0;
  const bool live = !__syncthreads_or(dup) && valid;
  const int j0 = (s * g.hs / IM_BANDS) * g.ws, j1 = ((s + 1) * g.hs / IM_BANDS) * g.ws;
  const size_t n_src = (size_t)g.ws * g.hs;
  double* out = edge_out + ((size_t)e * IM_BANDS + s) * IM_ROW;
  if (!live) {
    if (tid < IM_ROW) out[tid] = 0.0;
    if (assoc)
      for (int j = j0 + tid; j < j1; j += IM_THREADS) assoc[(size_t)e * n_src + j] = -1;
    return;
  }
  // R_ab = R_a^T R_b, t_ab = R_a^T (t_b - t_a)
  const double* Pa = poses + a * 16;
  const double* Pb = poses + b * 16;
  double Ra[9], ta[3], R[9], t[3];
  {
    double Rb[9], d[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) Ra[i * 3 + j] = Pa[i * 4 + j], Rb[i * 3 + j] = Pb[i * 4 + j];
      ta[i] = Pa[i * 4 + 3];
      d[i] = Pb[i * 4 + 3] - ta[i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) R[i * 3 + j] = (Ra[i] * Rb[j] + Ra[3 + i] * Rb[3 + j]) + Ra[6 + i] * Rb[6 + j];
      t[i] = (Ra[i] * d[0] + Ra[3 + i] * d[1]) + Ra[6 + i] * d[2];
    }
  }
  const EsCam ka = cams.k[a];
  const size_t hw = (size_t)g.H * g.W;
  const double* __restrict__ A = maps + (size_t)a * hw * 6;
  const double* __restrict__ B = maps + (size_t)b * hw * 6;
  double acc[IM_SUMS + 1];
#pragma unroll
  for (int i = 0; i <= IM_SUMS; ++i) acc[i] = 0.0;
#pragma unroll 1
  for (int j = j0 + tid; j < j1; j += IM_THREADS) {
    const int sy = j / g.ws, sx = j - sy * g.ws;
    const double* mb = B + ((size_t)(sy * g.stride) * g.W + sx * g.stride) * 6;
    const double mx = mb[3], my = mb[4], mz = mb[5];
    int q = -1;
    if (mx == mx) {   // B has a normal here: a usable source pixel
      acc[IM_SUMS] += 1.0;
      const double X[3] = {mb[0], mb[1], mb[2]};
      const double Px = (R[0] * X[0] + R[1] * X[1]) + R[2] * X[2], Py = (R[3] * X[0] + R[4] * X[1]) + R[5] * X[2],
                   Pz = (R[6] * X[0] + R[7] * X[1]) + R[8] * X[2];
      const double Yx = Px + t[0], Yy = Py + t[1], Yz = Pz + t[2];
      if (Yz > 0.0) {   // false for NaN
        const double xn = Yx / Yz, yn = Yy / Yz;
        const double u = rint((ka.fx * xn + ka.s * yn) + ka.cx), v = rint(ka.fy * yn + ka.cy);
        if (u >= 0.0 && u < (double)g.W && v >= 0.0 && v < (double)g.H) {
          const size_t qa = (size_t)(int)v * g.W + (int)u;
          const double* ma = A + qa * 6;
          const double nx = ma[3], ny = ma[4], nz = ma[5];
          if (nx == nx) {   // A has a normal there
            const double dx = Yx - ma[0], dy = Yy - ma[1], dz = Yz - ma[2];
            if ((dx * dx + dy * dy) + dz * dz <= g.max_d2) {
              const double Rx = (R[0] * mx + R[1] * my) + R[2] * mz, Ry = (R[3] * mx + R[4] * my) + R[5] * mz,
                           Rz = (R[6] * mx + R[7] * my) + R[8] * mz;
              if ((Rx * nx + Ry * ny) + Rz * nz >= g.normal_cos) {
                q = (int)qa;
                const double r = (nx * dx + ny * dy) + nz * dz;
                // into the world frame: N = R_a n_a, Yc = (R_a Y + t_a) - c; the row over view b's twist is (Yc x N, N)
                const double N0 = (Ra[0] * nx + Ra[1] * ny) + Ra[2] * nz, N1 = (Ra[3] * nx + Ra[4] * ny) + Ra[5] * nz,
                             N2 = (Ra[6] * nx + Ra[7] * ny) + Ra[8] * nz;
                const double C0 = (((Ra[0] * Yx + Ra[1] * Yy) + Ra[2] * Yz) + ta[0]) - g.c[0],
                             C1 = (((Ra[3] * Yx + Ra[4] * Yy) + Ra[5] * Yz) + ta[1]) - g.c[1],
                             C2 = (((Ra[6] * Yx + Ra[7] * Yy) + Ra[8] * Yz) + ta[2]) - g.c[2];
                const double J[6] = {C1 * N2 - C2 * N1, C2 * N0 - C0 * N2, C0 * N1 - C1 * N0, N0, N1, N2};
#pragma unroll
                for (int i = 0; i < 6; ++i) {
#pragma unroll
                  for (int k = i; k < 6; ++k) acc[rf_tri<6>(i, k)] += J[i] * J[k];
                  acc[21 + i] += J[i] * r;
                }
                acc[27] += r * r;
                acc[28] += 1.0;
              }
            }
          }
        }
      }
    }
    if (assoc) assoc[(size_t)e * n_src + j] = q;
  }
#pragma unroll
  for (int i = 0; i <= IM_SUMS; ++i) acc[i] = rs_wave_sum(acc[i]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int i = 0; i <= IM_SUMS; ++i) sh[tid >> 6][i] = acc[i];
  }
  __syncthreads();
  if (tid < IM_ROW) {
    double x = 0.0;
    if (tid <= IM_SUMS) {
      x = sh[0][tid];
      for (int w = 1; w < IM_THREADS / 64; ++w) x = x + sh[w][tid];
    }
    out[tid] = x;
  }
}

// entry i of edge e: its bands in band order
__device__ __forceinline__ double im_band_sum(const double* __restrict__ edge_out, int e, int i) {
  const double* p = edge_out + (size_t)e * IM_EDGE + i;
  double x = p[0];
  for (int s = 1; s < IM_BANDS; ++s) x = x + p[s * IM_ROW];
  return x;
}

// Evaluation k of the chain.  The system of the free views (slots in index order, 6 unknowns each: w, dt of the twist): block
// (v, v) = the sum of A over the kept edges that touch v, the other view ascending and (v, w) before (w, v); block (a, b) = -A
// of (a, b) and (b, a); the gradient +g at the source b and -g at the target a of every kept edge.
__global__ __launch_bounds__(IM_THREADS) void im_solve_kernel(int n, int E, const int32_t* __restrict__ edges, uint32_t fixed_mask,
                                                               const int32_t* __restrict__ found, double c0, double c1, double c2, double pivot_tol,
                                                               int k, int last, double* __restrict__ poses, const double* __restrict__ edge_out,
                                                               int32_t* __restrict__ info, int32_t* __restrict__ view_info,
                                                               double* __restrict__ stats, double* __restrict__ hist) {
  // rows 0 .. m-1: the system (lower triangle), row m: the right-hand side; 187 * 188 / 2 doubles
  __shared__ double L[(IM_MAX_DIM + 1) * (IM_MAX_DIM + 2) / 2];
  __shared__ double xs[IM_MAX_DIM + 6];
  __shared__ double diag0[IM_MAX_DIM + 6];
  __shared__ int16_t tab[IM_TAB];   // the kept edge of an ordered pair of views, or -1
  __shared__ int slot[TV_MAX_VIEWS], view_of[TV_MAX_VIEWS], vpairs[TV_MAX_VIEWS], vedges[TV_MAX_VIEWS], vfree[TV_MAX_VIEWS];
  __shared__ int tot_i[3];          // free views, pairs, kept edges
  __shared__ double tot_err;
  const int tid = threadIdx.x;
  if (info[3] != 0) {   // stopped at an earlier evaluation: uniform
    if (hist && tid < 4) hist[(size_t)k * 4 + tid] = 0.0;
    return;
  }
  for (int i = tid; i < IM_TAB; i += IM_THREADS) tab[i] = -1;
  __syncthreads();
  // the front of L, until the system is assembled: every edge's pairs, then every edge's squared error
  double* ep = L;
  double* er = L + 1024;
  for (int e = tid; e < E; e += IM_THREADS) {
    const double p = im_band_sum(edge_out, e, 28);
    ep[e] = p;
    er[e] = im_band_sum(edge_out, e, 27);
    const int a = edges[2 * e], b = edges[2 * e + 1];
    if (p >= (double)IM_MIN_PAIRS && a >= 0 && a < n && b >= 0 && b < n) tab[a * TV_MAX_VIEWS + b] = (int16_t)e;
  }
  __syncthreads();
  if (tid < TV_MAX_VIEWS) {
    int np = 0, ne = 0;
    if (tid < n)
      for (int w = 0; w < n; ++w) {
        const int e1 = tab[tid * TV_MAX_VIEWS + w], e2 = tab[w * TV_MAX_VIEWS + tid];
        if (e1 >= 0) np += (int)ep[e1], ++ne;
        if (e2 >= 0) np += (int)ep[e2], ++ne;
      }
    const bool is_free = tid < n && !(fixed_mask >> tid & 1u) && (!found || found[tid] != 0) && ne >= 1;
    const unsigned long long mask = __ballot(is_free);
    const int sl = is_free ? __popcll(mask & ((1ull << tid) - 1ull)) : -1;
    slot[tid] = sl;
    if (is_free) view_of[sl] = tid;
    vpairs[tid] = np, vedges[tid] = ne, vfree[tid] = is_free ? 1 : 0;
    if (tid == 0) tot_i[0] = __popcll(mask);
  } else if (tid == 64) {   // the kept edges in edge order
    int pairs = 0, kept = 0;
    double err = 0.0;
    for (int e = 0; e < E; ++e) {
      if (ep[e] >= (double)IM_MIN_PAIRS) pairs += (int)ep[e], ++kept, err = err + er[e];
    }
    tot_i[1] = pairs, tot_i[2] = kept, tot_err = err;
  }
  __syncthreads();
  const int F = tot_i[0], pairs = tot_i[1], kept = tot_i[2];
  const double err = tot_err;
  const int m = 6 * F;
  int reason = F == 0 || pairs < IM_MIN_PAIRS ? 1 : 0;
  double min_ratio = 0.0;
  bool stepped = false;
  __syncthreads();   // ep and er have been read: L may be written
  if (reason == 0 && !last) {
    const int nblk = F * (F + 1) / 2;
    int bad = fabs(err) < INFINITY ? 0 : 1;
    for (int it = tid; it < nblk * 36 + m; it += IM_THREADS) {
      double val = 0.0;
      if (it < nblk * 36) {
        const int blk = it / 36, i = it - blk * 36, r = i / 6, c = i - r * 6;
        int p = 0;
        while ((p + 1) * (p + 2) / 2 <= blk) ++p;
        const int q = blk - p * (p + 1) / 2;
        if (p == q && c > r) continue;
        const int v = view_of[p], w = view_of[q];   // v >= w
        const int t = r < c ? rf_tri<6>(r, c) : rf_tri<6>(c, r);
        if (p == q) {
          for (int u = 0; u < n; ++u) {
            const int e1 = tab[v * TV_MAX_VIEWS + u], e2 = tab[u * TV_MAX_VIEWS + v];
            if (e1 >= 0) val = val + im_band_sum(edge_out, e1, t);
            if (e2 >= 0) val = val + im_band_sum(edge_out, e2, t);
          }
          if (r == c) diag0[6 * p + r] = val;
        } else {
          const int e1 = tab[w * TV_MAX_VIEWS + v], e2 = tab[v * TV_MAX_VIEWS + w];
          double x = 0.0;
          if (e1 >= 0) x = x + im_band_sum(edge_out, e1, t);
          if (e2 >= 0) x = x + im_band_sum(edge_out, e2, t);
          val = -x;
        }
        L[ch_tri(6 * p + r, 6 * q + c)] = val;
      } else {
        const int i = it - nblk * 36, p = i / 6, r = i - p * 6, v = view_of[p];
        for (int u = 0; u < n; ++u) {
          const int e1 = tab[v * TV_MAX_VIEWS + u], e2 = tab[u * TV_MAX_VIEWS + v];
          if (e1 >= 0) val = val - im_band_sum(edge_out, e1, 21 + r);   // v is the target
          if (e2 >= 0) val = val + im_band_sum(edge_out, e2, 21 + r);   // v is the source
        }
        L[ch_tri(m, i)] = val;
      }
      if (!(fabs(val) < INFINITY)) bad = 1;   // also for NaN
    }
    if (__syncthreads_or(bad)) {
      reason = 3;
    } else {
      // Cholesky and both solves (chol.h); a pivot must be positive, finite and above pivot_tol of its entry before the elimination
      min_ratio = INFINITY;
      const bool fail = !ch_factor<IM_THREADS>(L, m, [&](int col, double pivot) {
        const double d0 = diag0[col];
        if (!(fabs(pivot) < INFINITY) || !(pivot > 0.0) || !(pivot > pivot_tol * d0)) return false;
        const double ratio = pivot / d0;
        if (ratio < min_ratio) min_ratio = ratio;
        return true;
      });
      if (fail) {
        reason = 2;
        min_ratio = 0.0;
      } else {
        ch_back<IM_THREADS>(L, m, xs);
        stepped = true;
        // the twist -x of every free view: R <- exp([w]x) R, t <- exp([w]x) (t - c) + c + dt
        if (tid < n && slot[tid] >= 0) {
          const double* x = xs + 6 * slot[tid];
          double* P = poses + tid * 16;
          const double w[3] = {-x[0], -x[1], -x[2]};
          double R[9], T[9];
          for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) R[i * 3 + j] = P[i * 4 + j], T[i * 3 + j] = 0.0;
          T[0] = P[3] - c0, T[3] = P[7] - c1, T[6] = P[11] - c2;
          rodrigues_rotate(w, R);
          rodrigues_rotate(w, T);
          for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) P[i * 4 + j] = R[i * 3 + j];
          P[3] = (T[0] + c0) - x[3], P[7] = (T[3] + c1) - x[4], P[11] = (T[6] + c2) - x[5];
        }
      }
    }
  }
  if (tid < n) {
    view_info[tid * 4] = vfree[tid], view_info[tid * 4 + 1] = vpairs[tid], view_info[tid * 4 + 2] = vedges[tid], view_info[tid * 4 + 3] = 0;
  }
  if (tid != 0) return;
  const int steps = info[1] + (stepped ? 1 : 0);
  info[0] = last && reason == 0 ? 1 : 0;
  info[1] = steps, info[2] = pairs, info[3] = reason, info[5] = kept, info[6] = F, info[7] = 0;
  stats[0] = err;
  stats[1] = pairs > 0 ? sqrt(err / (double)pairs) : 0.0;
  if (hist) {
    double* h = hist + (size_t)k * 4;
    h[0] = err, h[1] = (double)pairs, h[2] = min_ratio, h[3] = 0.0;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
namespace {

const char* im_shape(int n, int lo, int H, int W) {
  if (n < lo || n > TV_MAX_VIEWS) return lo == 1 ? "n must be in [1, 32]" : "n must be in [2, 32]";
  if (H < 3 || W < 3 || (long long)n * H * W > MAX_PIXELS) return "H and W must be >= 3 with at most 2^28 pixels in all";
  return nullptr;
}

}  // namespace

extern "C" {

int cotr_icp_maps(const float* depths, int n, int H, int W, const double* Ks, double edge, double* maps_out, int32_t* info_out, cotr_stream stream) {
  static const char* const FN = "cotr_icp_maps";
  if (const char* what = im_shape(n, 1, H, W)) return arg_fail(FN, what);
  if (!(edge > 0.0) || !(edge < INFINITY)) return arg_fail(FN, "edge must be finite and > 0");
  if (!depths || !Ks || !maps_out || !info_out) return arg_fail(FN, "depths, Ks, maps_out and info_out must not be NULL");
  EsCams cams;
  if (const char* what = es_cameras(Ks, n, &cams)) return arg_fail(FN, what);
  if (!aligned(depths, 4) || !aligned(maps_out, 8) || !aligned(info_out, 4)) return arg_fail(FN, "floats and int32 must be 4-byte and doubles 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(im_maps_begin_kernel, dim3(1), dim3(64), 0, s, n, info_out);
  hipLaunchKernelGGL(im_map_kernel, dim3((unsigned)((H * W + 255) / 256), (unsigned)n), dim3(256), 0, s, depths, H, W, cams, edge, maps_out, info_out);
  return launched();
}

int cotr_icp_multiview(const double* maps, int n, int H, int W, const double* Ks, const double* c2w0, const int32_t* edges, int E,
                       uint32_t fixed_mask, const double* centre, const int32_t* found, double max_dist, double normal_cos, double pivot_tol,
                       int iters, int stride, double* c2w_out, int32_t* info_out, int32_t* view_info_out, double* stats_out, double* edge_out,
                       double* hist_out, int32_t* assoc_out, cotr_stream stream) {
  static const char* const FN = "cotr_icp_multiview";
  if (const char* what = im_shape(n, 2, H, W)) return arg_fail(FN, what);
  if (E < 1 || E > n * (n - 1)) return arg_fail(FN, "E must be in [1, n (n - 1)]");
  if (!(fixed_mask & (n == 32 ? 0xFFFFFFFFu : (1u << n) - 1u))) return arg_fail(FN, "fixed_mask must fix at least one of the n views");
  if (iters < 0 || iters > IM_MAX_ITERS) return arg_fail(FN, "iters must be in [0, 64]");
  if (stride < 1 || stride > IM_MAX_STRIDE) return arg_fail(FN, "stride must be in [1, 64]");
  if (!(max_dist > 0.0) || !(max_dist < INFINITY)) return arg_fail(FN, "max_dist must be finite and > 0");
  if (!(normal_cos >= -1.0) || !(normal_cos <= 1.0)) return arg_fail(FN, "normal_cos must be in [-1, 1]");
  if (!(pivot_tol > 0.0) || !(pivot_tol < 1.0)) return arg_fail(FN, "pivot_tol must be in (0, 1)");
  if (!maps || !Ks || !c2w0 || !edges || !centre || !c2w_out || !info_out || !view_info_out || !stats_out || !edge_out)
    return arg_fail(FN, "maps, Ks, c2w0, edges, centre, c2w_out, info_out, view_info_out, stats_out and edge_out must not be NULL");
  EsCams cams;
  if (const char* what = es_cameras(Ks, n, &cams)) return arg_fail(FN, what);
  if (!isfinite(centre[0]) || !isfinite(centre[1]) || !isfinite(centre[2])) return arg_fail(FN, "centre must be finite");
  if (!aligned(maps, 8) || !aligned(c2w0, 8) || !aligned(edges, 4) || !aligned(found, 4) || !aligned(c2w_out, 8) || !aligned(info_out, 4) ||
      !aligned(view_info_out, 4) || !aligned(stats_out, 8) || !aligned(edge_out, 8) || !aligned(hist_out, 8) || !aligned(assoc_out, 4))
    return arg_fail(FN, "int32 must be 4-byte and doubles 8-byte aligned");
  ImGrid g;
  g.n = n, g.H = H, g.W = W, g.stride = stride;
  g.ws = (W + stride - 1) / stride, g.hs = (H + stride - 1) / stride;
  g.max_d2 = max_dist * max_dist, g.normal_cos = normal_cos;
  g.c[0] = centre[0], g.c[1] = centre[1], g.c[2] = centre[2];
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(im_begin_kernel, dim3(1), dim3(IM_THREADS), 0, s, n, E, c2w0, edges, found, c2w_out, info_out, view_info_out, stats_out);
  for (int k = 0; k <= iters; ++k) {
    hipLaunchKernelGGL(im_edge_kernel, dim3(IM_BANDS, (unsigned)E), dim3(IM_THREADS), 0, s, maps, cams, g, edges, found, (const double*)c2w_out,
                       (const int32_t*)info_out, edge_out, assoc_out);
    hipLaunchKernelGGL(im_solve_kernel, dim3(1), dim3(IM_THREADS), 0, s, n, E, edges, fixed_mask, found, g.c[0], g.c[1], g.c[2], pivot_tol, k,
                       (int)(k == iters), c2w_out, (const double*)edge_out, info_out, view_info_out, stats_out, hist_out);
  }
  return launched();
}

}  // extern "C"
