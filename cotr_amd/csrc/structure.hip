// Structure from known cameras: cotr_triangulate_views, robust N-view triangulation of correspondences seen in 2 to 32 posed
// views.  Handle-less (handleless.h), stream-ordered, integer atomics only, every point summed by one thread
// in one order: the same input gives the same bits.  Compiled with -ffp-contract=off.
//
//   1. tv_prepare_kernel  a thread per view: camera, pose, centre c = -R^T t and the view's validity -> the view table in
//                         scratch; the counters zeroed, info[0] = found
//   2. tv_points_kernel   a thread per point; the view table in LDS, read at uniform addresses; the pixels of a view are read
//                         coalesced from points [V, N, 2] whenever a loop needs them (nothing per view lives in registers)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "handleless.h"
#include "view_table.h"

using namespace cotr_detail;

#define TV_MAX_POINTS (1 << 24)
#define TV_MAX_REFINE 64
#define TV_THREADS 64

// ---- per-view arithmetic (w: the view's row of the table; the pixel, its ray, the projection and the solve are in view_table.h) -----
// d = tv_view_ray, normalised
__device__ __forceinline__ void tv_ray(const double* w, const TvPixel& q, double* d) {
  double r[3];
  tv_view_ray(w, q.u, q.v, r);
  const double len = sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
  d[0] = r[0] / len, d[1] = r[1] / len, d[2] = r[2] / len;
}

// acc[0..5] += I - d d^T (00 01 02 11 12 22), acc[6..8] += (I - d d^T) c = c - d (d . c)
__device__ __forceinline__ void tv_accum(const double* w, const TvPixel& q, double* acc) {
  double d[3];
  tv_ray(w, q, d);
  const double* c = w + TV_C;
  acc[0] += 1.0 - d[0] * d[0];
  acc[1] -= d[0] * d[1];
  acc[2] -= d[0] * d[2];
  acc[3] += 1.0 - d[1] * d[1];
  acc[4] -= d[1] * d[2];
  acc[5] += 1.0 - d[2] * d[2];
  const double dc = (d[0] * c[0] + d[1] * c[1]) + d[2] * c[2];
  acc[6] += c[0] - d[0] * dc;
  acc[7] += c[1] - d[1] * dc;
  acc[8] += c[2] - d[2] * dc;
}

// ---- per-point loops over a set of views (a bit mask), ascending ----------------------------------------------------------
struct TvPoint {
  const double* tab;                    // the view table in LDS
  const double* __restrict__ points;
  size_t N, p;
  int V;
};

// ray least squares over the views of `set` -> X; false: degenerate
__device__ bool tv_rays_point(const TvPoint& c, uint32_t set, double* X) {
  double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int v = 0; v < c.V; ++v)
    if (set >> v & 1u) tv_accum(c.tab + v * TV_ROW, tv_pixel(c.points, c.N, v, c.p), acc);
  return tv_solve(acc, acc + 6, X);
}

// The summed squared error of X over `set`, whether every view has depth > 0, and the Gauss-Newton system:
// A (00 01 02 11 12 22) = sum ju ju^T + jv jv^T, g = sum ju du + jv dv, (ju, jv) the rows of d(u, v) / dX.
__device__ void tv_normal(const TvPoint& c, uint32_t set, const double* X, double* err, bool* front, double* A, double* g) {
  double e = 0.0;
  bool f = true;
#pragma unroll
  for (int i = 0; i < 6; ++i) A[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) g[i] = 0.0;
  for (int v = 0; v < c.V; ++v) {
    if (!(set >> v & 1u)) continue;
    const double* w = c.tab + v * TV_ROW;
    const TvProj r = tv_project(w, tv_pixel(c.points, c.N, v, c.p), X);
    e += r.e;
    f = f && r.z > 0.0;
    const double* R = w + TV_R;
    double ju[3], jv[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double a = (R[k] - r.xn * R[6 + k]) / r.z, b = (R[3 + k] - r.yn * R[6 + k]) / r.z;
      ju[k] = w[0] * a + w[4] * b;
      jv[k] = w[1] * b;
    }
    A[0] += ju[0] * ju[0] + jv[0] * jv[0];
    A[1] += ju[0] * ju[1] + jv[0] * jv[1];
    A[2] += ju[0] * ju[2] + jv[0] * jv[2];
    A[3] += ju[1] * ju[1] + jv[1] * jv[1];
    A[4] += ju[1] * ju[2] + jv[1] * jv[2];
    A[5] += ju[2] * ju[2] + jv[2] * jv[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] += ju[k] * r.du + jv[k] * r.dv;
  }
  *err = e;
  *front = f;
}

// ---- kernels --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TV_THREADS) void tv_points_kernel(const double* __restrict__ points, const uint8_t* __restrict__ visible,
                                                               int V, int n, const double* __restrict__ tab_in,
                                                               const int32_t* __restrict__ found, float thr, double max_cos, double dist,
                                                               int refine_iters, int robust, int rule, double* __restrict__ X_out,
                                                               uint8_t* __restrict__ used, double* __restrict__ quality,
                                                               uint8_t* __restrict__ mask, int32_t* __restrict__ info) {
  __shared__ double tab[TV_MAX_VIEWS * TV_ROW];
  for (int i = threadIdx.x; i < V * TV_ROW; i += TV_THREADS) tab[i] = tab_in[i];
  __syncthreads();
  const size_t N = (size_t)n;
  const size_t p = (size_t)blockIdx.x * TV_THREADS + threadIdx.x;
  if (p >= N) return;
  if (found && found[0] == 0) {
    for (int i = 0; i < 3; ++i) X_out[p * 3 + i] = 0.0;
    for (int i = 0; i < 5; ++i) quality[p * 5 + i] = 0.0;
    for (int v = 0; v < V; ++v) used[(size_t)v * N + p] = 0;
    mask[p] = 0;
    return;
  }
  const TvPoint c = {tab, points, N, p, V};

  // S: the visible views with finite coordinates
  uint32_t S = 0;
  for (int v = 0; v < V; ++v) {
    const bool vis = visible ? visible[(size_t)v * N + p] != 0 : true;
    if (vis && tab[v * TV_ROW + TV_OK] != 0.0 && tv_pixel(points, N, v, p).finite) S |= 1u << v;
  }

  uint32_t U = S;
  bool enough = __popc(S) >= 2;
  if (enough && robust) {
    // every pair i < j of S: the first with the most views in front and within the threshold
    int best = 0;
    U = 0;
    for (int i = 0; i < V; ++i) {
      if (!(S >> i & 1u)) continue;
      for (int j = i + 1; j < V; ++j) {
        if (!(S >> j & 1u)) continue;
        double Xp[3];
        if (!tv_rays_point(c, 1u << i | 1u << j, Xp)) continue;
        uint32_t in = 0;
        for (int v = 0; v < V; ++v) {
          if (!(S >> v & 1u)) continue;
          const TvProj r = tv_project(tab + v * TV_ROW, tv_pixel(points, N, v, p), Xp);
          if (r.z > 0.0 && (float)r.e <= thr) in |= 1u << v;
        }
        const int cnt = __popc(in);
        if (cnt > best) best = cnt, U = in;
      }
    }
    enough = best >= 2;
  }

  double X[3] = {0.0, 0.0, 0.0};
  bool solved = false;
  int kept = 0;
  if (enough) {
    if (rule == 1) {
      // the point on ray A nearest ray B: X = c_a + s d_a, s = (d_a.w - (d_a.d_b)(d_b.w)) / (1 - (d_a.d_b)^2), w = c_b - c_a
      double da[3], db[3];
      tv_ray(tab, tv_pixel(points, N, 0, p), da);
      tv_ray(tab + TV_ROW, tv_pixel(points, N, 1, p), db);
      const double* ca = tab + TV_C;
      const double* cb = tab + TV_ROW + TV_C;
      const double w0 = cb[0] - ca[0], w1 = cb[1] - ca[1], w2 = cb[2] - ca[2];
      const double ab = (da[0] * db[0] + da[1] * db[1]) + da[2] * db[2];
      const double aw = (da[0] * w0 + da[1] * w1) + da[2] * w2, bw = (db[0] * w0 + db[1] * w1) + db[2] * w2;
      const double den = 1.0 - ab * ab;
      const double s = (aw - ab * bw) / den;
      X[0] = ca[0] + s * da[0], X[1] = ca[1] + s * da[1], X[2] = ca[2] + s * da[2];
      solved = den != 0.0 && isfinite(den) && isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]);
    } else {
      solved = tv_rays_point(c, U, X);
      if (solved && refine_iters > 0) {
        double err, A[6], g[3];
        bool front;
        tv_normal(c, U, X, &err, &front, A, g);
        for (int it = 0; front && it < refine_iters; ++it) {
          double step[3];
          if (!tv_solve(A, g, step)) break;
          const double Xn[3] = {X[0] - step[0], X[1] - step[1], X[2] - step[2]};
          double err_n, An[6], gn[3];
          bool front_n;
          tv_normal(c, U, Xn, &err_n, &front_n, An, gn);
          if (!(front_n && err_n < err)) break;
          X[0] = Xn[0], X[1] = Xn[1], X[2] = Xn[2];
          err = err_n;
#pragma unroll
          for (int i = 0; i < 6; ++i) A[i] = An[i];
#pragma unroll
          for (int i = 0; i < 3; ++i) g[i] = gn[i];
          ++kept;
        }
      }
    }
  }

  if (!solved) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int i = 0; i < 3; ++i) X_out[p * 3 + i] = nan;
    for (int i = 0; i < 5; ++i) quality[p * 5 + i] = nan;
    for (int v = 0; v < V; ++v) used[(size_t)v * N + p] = 0;
    mask[p] = 0;
    atomicAdd(info + (enough ? 3 : 2), 1);
    return;
  }

  // quality over U at X
  double sum = 0.0, emax = 0.0, zmin = INFINITY, zmax = -INFINITY, cmin = INFINITY;
  bool depth_ok = true, err_ok = true;
  for (int v = 0; v < V; ++v) {
    if (!(U >> v & 1u)) continue;
    const TvProj r = tv_project(tab + v * TV_ROW, tv_pixel(points, N, v, p), X);
    sum += r.e;
    emax = r.e > emax ? r.e : emax;
    zmin = r.z < zmin ? r.z : zmin;
    zmax = r.z > zmax ? r.z : zmax;
    depth_ok = depth_ok && r.z > 0.0 && r.z < dist;
    err_ok = err_ok && (float)r.e <= thr;
  }
  for (int i = 0; i < V; ++i) {
    if (!(U >> i & 1u)) continue;
    double di[3];
    tv_ray(tab + i * TV_ROW, tv_pixel(points, N, i, p), di);
    for (int j = i + 1; j < V; ++j) {
      if (!(U >> j & 1u)) continue;
      double dj[3];
      tv_ray(tab + j * TV_ROW, tv_pixel(points, N, j, p), dj);
      const double cs = (di[0] * dj[0] + di[1] * dj[1]) + di[2] * dj[2];
      cmin = cs < cmin ? cs : cmin;
    }
  }
  const bool par_ok = cmin <= max_cos;
  const bool good = depth_ok && err_ok && par_ok;
  for (int i = 0; i < 3; ++i) X_out[p * 3 + i] = X[i];
  double* q = quality + p * 5;
  q[0] = sum / (double)__popc(U), q[1] = emax, q[2] = zmin, q[3] = zmax, q[4] = cmin;
  for (int v = 0; v < V; ++v) used[(size_t)v * N + p] = (uint8_t)(U >> v & 1u);
  mask[p] = good ? 1 : 0;
  atomicAdd(info + (good ? 1 : !depth_ok ? 4 : !err_ok ? 5 : 6), 1);
  if (kept) atomicAdd(info + 7, kept);
}

// ---- host side ------------------------------------------------------------------------------------------------------------
namespace {

size_t tv_scratch_bytes() { return align_up((size_t)TV_MAX_VIEWS * TV_ROW * sizeof(double)); }

const char* const TV_FN = "cotr_triangulate_views";

const char* tv_check_shape(int V, int n) {
  if (V < 2 || V > TV_MAX_VIEWS) return "V must be in [2, 32]";
  if (n < 1 || n > TV_MAX_POINTS) return "n must be in [1, 2^24]";
  return nullptr;
}

}  // namespace

extern "C" {

int cotr_triangulate_views_scratch_bytes(int V, int n, size_t* bytes) {
  if (!bytes) return arg_fail("cotr_triangulate_views_scratch_bytes", "bytes is NULL");
  if (const char* msg = tv_check_shape(V, n)) return arg_fail(TV_FN, msg);
  *bytes = tv_scratch_bytes();
  return COTR_OK;
}

int cotr_triangulate_views(const double* points, const uint8_t* visible, const double* cams, const double* poses, int V, int n,
                           const int32_t* found, double threshold, double max_cos, double distance_thresh, int refine_iters, int robust,
                           int rule, double* X_out, uint8_t* used_out, double* quality_out, uint8_t* mask_out, int32_t* info_out,
                           void* scratch, size_t scratch_bytes, cotr_stream stream) {
  if (const char* msg = tv_check_shape(V, n)) return arg_fail(TV_FN, msg);
  if (!(threshold > 0.0) || !(threshold < INFINITY)) return arg_fail(TV_FN, "threshold must be finite and > 0");
  const float thr = (float)(threshold * threshold);
  if (!(thr > 0.0f) || !(thr < INFINITY))
    return arg_fail(TV_FN, "the squared threshold must be a finite float32 that is not 0");
  if (!(max_cos >= -1.0) || !(max_cos <= 1.0)) return arg_fail(TV_FN, "max_cos must be in [-1, 1]");
  if (!(distance_thresh > 0.0) || !(distance_thresh < INFINITY))
    return arg_fail(TV_FN, "distance_thresh must be finite and > 0");
  if (refine_iters < 0 || refine_iters > TV_MAX_REFINE) return arg_fail(TV_FN, "refine_iters must be in [0, 64]");
  if (robust != 0 && robust != 1) return arg_fail(TV_FN, "robust must be 0 or 1");
  if (rule != 0 && rule != 1) return arg_fail(TV_FN, "rule must be 0 (rays) or 1 (demo)");
  if (rule == 1 && (V != 2 || robust != 0 || refine_iters != 0))
    return arg_fail(TV_FN, "rule 1 (demo) takes V = 2, robust = 0 and refine_iters = 0");
  if (!points || !cams || !poses || !X_out || !used_out || !quality_out || !mask_out || !info_out || !scratch)
    return arg_fail(TV_FN, "points, cams, poses, X_out, used_out, quality_out, mask_out, info_out and scratch must not be NULL");
  if (!aligned(points, 16) || !aligned(cams, 8) || !aligned(poses, 8) || !aligned(X_out, 8) || !aligned(quality_out, 8) ||
      !aligned(info_out, 4) || !aligned(found, 4) || !aligned(scratch, 16))
    return arg_fail(TV_FN, "points and scratch must be 16-byte, other doubles 8-byte and ints 4-byte aligned");
  if (scratch_bytes < tv_scratch_bytes()) return arg_fail(TV_FN, "scratch is smaller than cotr_triangulate_views_scratch_bytes");
  double* tab = static_cast<double*>(scratch);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(tv_prepare_kernel, dim3(1), dim3(64), 0, s, cams, poses, V, found, tab, info_out);
  hipLaunchKernelGGL(tv_points_kernel, dim3((unsigned)((n + TV_THREADS - 1) / TV_THREADS)), dim3(TV_THREADS), 0, s, points, visible, V, n, tab,
                     found, thr, max_cos, distance_thresh, refine_iters, robust, rule, X_out, used_out, quality_out, mask_out, info_out);
  return launched();
}

}  // extern "C"
