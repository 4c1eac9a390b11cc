// Multi-view depth maps: cotr_corr_depth, the depth map of a reference view from its correspondence maps into
// 1 to 31 posed neighbour views, and cotr_depth_consistency, the cross-check of 2 to 32 depth maps of one size against each other.
// Handle-less (handleless.h), stream-ordered, no scratch, integer atomics only, every pixel summed by one thread in one order: the
// same input gives the same bits.  Compiled with -ffp-contract=off.
//
// cotr_corr_depth
//   1. hl_begin_kernel        (handleless.h) info = {found, 0, ...}
//   2. md_depth_kernel        a thread per pixel.  Every workgroup rebuilds the view table (tv_view_row of view_table.h: the Prepare rule of
//                             cotr_triangulate_views, at most 32 x 24 doubles) in LDS with a thread per view and reads it at uniform
//                             addresses; the 8 bytes of a neighbour's correspondence are read coalesced whenever a loop needs them
//                             (nothing per view lives in registers: the sets of views are 32-bit masks)
// cotr_depth_consistency
//   1. hl_begin_kernel        info[i] = {found[i], 0, 0, 0}
//   2. md_consistency_kernel  grid (blocks of pixels, n): the reference view is blockIdx.y, so its camera and pose are wave-uniform;
//                             the depth of view j at the projected pixel is the only gather
// The counters of both are wave ballots, summed per workgroup in LDS, one integer atomic a counter and workgroup.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "handleless.h"
#define TV_NO_PREPARE_KERNEL   // the table is built in LDS by every workgroup: tv_view_row alone
#include "view_table.h"

using namespace cotr_detail;

#define MD_THREADS 256
#define MD_WAVES (MD_THREADS / 64)
#define MD_MAX_REFINE 64
#define MD_MAX_MAPS ES_MAX_CAMS

// per-wavefront counts -> part[wave][col]; then, after a barrier, one atomic a column whose sum is not 0: column i goes to dst[i],
// from column `gap` on to dst[i + 1]
template <int COLS>
__device__ __forceinline__ void md_flush(int (*part)[COLS], const int* mine, int32_t* __restrict__ dst, int gap = COLS) {
  if ((threadIdx.x & 63) == 0)
    for (int i = 0; i < COLS; ++i) part[threadIdx.x >> 6][i] = mine[i];
  __syncthreads();
  if (threadIdx.x < COLS) {
    int s = 0;
#pragma unroll
    for (int k = 0; k < MD_WAVES; ++k) s += part[k][threadIdx.x];
    if (s) atomicAdd(dst + threadIdx.x + ((int)threadIdx.x >= gap ? 1 : 0), s);
  }
}

// ---- cotr_corr_depth --------------------------------------------------------------------------------------------------------
struct MdPixel {
  const double* tab;                 // the view table in LDS
  const float* __restrict__ corr;
  size_t HW, p;
  int V;
  double r[3];                       // the reference ray
};

// what neighbour view j >= 1 (map j - 1) says of the pixel
__device__ __forceinline__ TvPixel md_pixel(const MdPixel& c, int j) {
  const float2 q = *reinterpret_cast<const float2*>(c.corr + ((size_t)(j - 1) * c.HW + c.p) * 2);
  return {(double)q.x, (double)q.y, isfinite(q.x) && isfinite(q.y)};
}

__device__ __forceinline__ void md_point(const MdPixel& c, double s, double* X) {
  const double* c0 = c.tab + TV_C;
  X[0] = c0[0] + s * c.r[0], X[1] = c0[1] + s * c.r[1], X[2] = c0[2] + s * c.r[2];
}

struct MdCand {
  bool parallax, ok;
  double s;
};

// the parameter of the point of the reference ray nearest the ray of view j
__device__ __forceinline__ MdCand md_candidate(const MdPixel& c, int j, const TvPixel& q, double max_cos) {
  const double* w = c.tab + j * TV_ROW;
  double rk[3];
  tv_view_ray(w, q.u, q.v, rk);
  const double* r = c.r;
  const double a = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
  const double b = (r[0] * rk[0] + r[1] * rk[1]) + r[2] * rk[2];
  const double e = (rk[0] * rk[0] + rk[1] * rk[1]) + rk[2] * rk[2];
  const double w0 = w[TV_C] - c.tab[TV_C], w1 = w[TV_C + 1] - c.tab[TV_C + 1], w2 = w[TV_C + 2] - c.tab[TV_C + 2];
  const double rw = (r[0] * w0 + r[1] * w1) + r[2] * w2, kw = (rk[0] * w0 + rk[1] * w1) + rk[2] * w2;
  const double den = a * e - b * b;
  MdCand o;
  o.s = (rw * e - b * kw) / den;
  o.parallax = b / sqrt(a * e) <= max_cos;   // false for NaN
  o.ok = den != 0.0 && isfinite(den) && isfinite(o.s) && o.s > 0.0;
  return o;
}

// E(s) over the views of U, whether every one keeps z > 0, and the scalar Gauss-Newton system A, g
__device__ void md_normal(const MdPixel& c, uint32_t U, double s, double* err, bool* front, double* A_out, double* g_out) {
  double X[3];
  md_point(c, s, X);
  double e = 0.0, A = 0.0, g = 0.0;
  bool f = true;
  for (int j = 1; j < c.V; ++j) {
    if (!(U >> j & 1u)) continue;
    const double* w = c.tab + j * TV_ROW;
    const TvProj pr = tv_project(w, md_pixel(c, j), X);
    e += pr.e;
    f = f && pr.z > 0.0;
    const double* R = w + TV_R;
    const double q0 = (R[0] * c.r[0] + R[1] * c.r[1]) + R[2] * c.r[2];
    const double q1 = (R[3] * c.r[0] + R[4] * c.r[1]) + R[5] * c.r[2];
    const double q2 = (R[6] * c.r[0] + R[7] * c.r[1]) + R[8] * c.r[2];
    const double a = (q0 - pr.xn * q2) / pr.z, b = (q1 - pr.yn * q2) / pr.z;
    const double ju = w[0] * a + w[4] * b, jv = w[1] * b;
    A += ju * ju + jv * jv;
    g += ju * pr.du + jv * pr.dv;
  }
  *err = e, *front = f, *A_out = A, *g_out = g;
}

__global__ __launch_bounds__(MD_THREADS) void md_depth_kernel(const float* __restrict__ corr, const uint8_t* __restrict__ valid,
                                                              const double* __restrict__ cams, const double* __restrict__ poses, int V, int H,
                                                              int W, const int32_t* __restrict__ found, float thr, double max_cos, double dist,
                                                              int min_views, int refine_iters, float* __restrict__ depth_out,
                                                              uint8_t* __restrict__ views_out, float* __restrict__ err_out,
                                                              int32_t* __restrict__ info) {
  __shared__ double tab[TV_MAX_VIEWS * TV_ROW];
  __shared__ int part[MD_WAVES][6];
  if ((int)threadIdx.x < V) tv_view_row(cams, poses, threadIdx.x, tab + threadIdx.x * TV_ROW);
  __syncthreads();
  const size_t HW = (size_t)H * W;
  const size_t p = (size_t)blockIdx.x * MD_THREADS + threadIdx.x;
  const bool in = p < HW;
  const bool on = (found ? found[0] != 0 : true) && tab[TV_OK] != 0.0;   // uniform
  if (!on) {
    if (in) depth_out[p] = 0.0f, views_out[p] = 0, err_out[p] = __builtin_nanf("");
    return;
  }

  // what: 0 a depth, 1 too few views, 2 no candidate, 3 dropped by depth, 4 dropped by error; -1 past the map
  int what = -1, kept = 0, nviews = 0;
  float depth = 0.0f, mean = __builtin_nanf("");
  if (in) {
    MdPixel c = {tab, corr, HW, p, V, {0.0, 0.0, 0.0}};
    tv_view_ray(tab, (double)(int)(p % (size_t)W), (double)(int)(p / (size_t)W), c.r);

    // P: the neighbours that see the pixel and have parallax; whether one of them gives a candidate
    uint32_t P = 0;
    bool any = false;
    for (int j = 1; j < V; ++j) {
      const bool vis = valid ? valid[(size_t)(j - 1) * HW + p] != 0 : true;
      if (!(vis && tab[j * TV_ROW + TV_OK] != 0.0)) continue;
      const TvPixel q = md_pixel(c, j);
      if (!q.finite) continue;
      const MdCand k = md_candidate(c, j, q, max_cos);
      if (!k.parallax) continue;
      P |= 1u << j;
      any = any || k.ok;
    }

    // the vote: candidates ascending, the first with the most views in front and within the threshold
    uint32_t U = 0;
    int best = 0;
    double s = 0.0;
    for (int k = 1; k < V; ++k) {
      if (!(P >> k & 1u)) continue;
      const MdCand cand = md_candidate(c, k, md_pixel(c, k), max_cos);
      if (!cand.ok) continue;
      double X[3];
      md_point(c, cand.s, X);
      uint32_t inl = 0;
      for (int j = 1; j < V; ++j) {
        if (!(P >> j & 1u)) continue;
        const TvProj pr = tv_project(tab + j * TV_ROW, md_pixel(c, j), X);
        if (pr.z > 0.0 && (float)pr.e <= thr) inl |= 1u << j;
      }
      const int cnt = __popc(inl);
      if (cnt > best) best = cnt, U = inl, s = cand.s;
    }

    if (!any) {
      what = 2;
    } else if (best < min_views) {
      what = 1;
    } else {
      double err, A, g;
      bool front;
      md_normal(c, U, s, &err, &front, &A, &g);
      for (int it = 0; front && it < refine_iters; ++it) {
        if (!(A > 0.0 && A < INFINITY)) break;
        const double sn = s - g / A;
        if (!(sn > 0.0)) break;
        double err_n, An, gn;
        bool front_n;
        md_normal(c, U, sn, &err_n, &front_n, &An, &gn);
        if (!(front_n && err_n < err)) break;
        s = sn, err = err_n, A = An, g = gn;
        ++kept;
      }
      // the filters at the final s
      double X[3];
      md_point(c, s, X);
      bool err_ok = true;
      for (int j = 1; j < V; ++j) {
        if (!(U >> j & 1u)) continue;
        const TvProj pr = tv_project(tab + j * TV_ROW, md_pixel(c, j), X);
        err_ok = err_ok && (float)pr.e <= thr;
      }
      const bool depth_ok = s > 0.0 && s < dist;
      what = !depth_ok ? 3 : !err_ok ? 4 : 0;
      if (what == 0) depth = (float)s, nviews = best, mean = (float)(err / (double)best);
    }
    depth_out[p] = depth, views_out[p] = (uint8_t)nviews, err_out[p] = mean;
  }

  int mine[6];
#pragma unroll
  for (int i = 0; i < 5; ++i) mine[i] = __popcll(__ballot(what == i));
  for (int o = 32; o > 0; o >>= 1) kept += __shfl_down(kept, o);
  mine[5] = kept;   // lane 0: the wavefront's steps
  md_flush<6>(part, mine, info + 1, 5);   // info[1..5] the five verdicts, info[7] the steps
}

// ---- cotr_depth_consistency -------------------------------------------------------------------------------------------------
// the camera and pose rules are pinhole.h's: es_vertex, es_to_world, es_to_camera, es_project, es_nearest
__global__ __launch_bounds__(MD_THREADS) void md_consistency_kernel(const float* __restrict__ depths, int n, int H, int W, EsCams cams,
                                                                    const double* __restrict__ c2w, const int32_t* __restrict__ found,
                                                                    const uint8_t* __restrict__ pairs, double px2, double rel, int min_views,
                                                                    int max_violations, float* __restrict__ depth_out,
                                                                    uint8_t* __restrict__ count_out, int32_t* __restrict__ info) {
  __shared__ int part[MD_WAVES][3];
  const int i = blockIdx.y;
  const size_t HW = (size_t)H * W;
  const size_t p = (size_t)blockIdx.x * MD_THREADS + threadIdx.x;
  const bool in = p < HW;
  if (found && found[i] == 0) {   // uniform
    if (in) depth_out[(size_t)i * HW + p] = 0.0f, count_out[(size_t)i * HW + p] = 0;
    return;
  }
  const EsCam ki = cams.k[i];
  const double* mi = c2w + i * 16;
  const int x = (int)(p % (size_t)W), y = (int)(p / (size_t)W);
  double Y[3], P[3] = {0.0, 0.0, 0.0};
  const bool ok = in && es_vertex(depths + (size_t)i * HW, W, ki, x, y, Y);
  if (ok) es_to_world(mi, Y, P);
  const double z = ok ? Y[2] : 0.0;
  int consistent = 0, violations = 0;
  double sum = z;
  for (int j = 0; j < n; ++j) {
    if (j == i || (found && found[j] == 0) || (pairs && pairs[i * n + j] == 0)) continue;   // uniform
    if (!ok) continue;
    const EsCam kj = cams.k[j];
    const double* mj = c2w + j * 16;
    double Pj[3], u, v;   // P in view j
    es_to_camera(mj, P, Pj);
    int xj, yj;
    if (!es_project(kj, Pj, &u, &v) || !es_nearest(u, v, H, W, &xj, &yj)) continue;
    double Yj[3], Q[3], Qi[3];   // the vertex of j there, in the world, back in view i
    if (!es_vertex(depths + (size_t)j * HW, W, kj, xj, yj, Yj)) continue;
    es_to_world(mj, Yj, Q);
    es_to_camera(mi, Q, Qi);
    bool good = es_project(ki, Qi, &u, &v);
    if (good) {
      const double du = u - (double)x, dv = v - (double)y;
      good = du * du + dv * dv <= px2 && fabs(Qi[2] - z) <= rel * z;
    }
    if (good)
      ++consistent, sum += Qi[2];
    else if (Yj[2] > Pj[2] * (1.0 + rel))
      ++violations;
  }
  const bool enough = ok && consistent >= min_views;
  const bool seen_through = enough && max_violations >= 0 && violations > max_violations;
  const bool keep = enough && !seen_through;
  if (in) {
    depth_out[(size_t)i * HW + p] = keep ? (float)(sum / (double)(1 + consistent)) : 0.0f;
    count_out[(size_t)i * HW + p] = (uint8_t)consistent;
  }
  const int mine[3] = {(int)__popcll(__ballot(ok)), (int)__popcll(__ballot(keep)), (int)__popcll(__ballot(seen_through))};
  md_flush<3>(part, mine, info + i * 4 + 1);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
namespace {

bool md_finite(double v) { return v > -INFINITY && v < INFINITY; }

// do [a, a + na) and [b, b + nb) share a byte (a NULL range shares none)
bool md_overlap(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b) return false;
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

struct MdRange {
  const void* p;
  size_t bytes;
};

// the first `outs` ranges are written: none of them may share a byte with any other range
bool md_alias(const MdRange* r, int count, int outs) {
  for (int a = 0; a < outs; ++a)
    for (int b = a + 1; b < count; ++b)
      if (md_overlap(r[a].p, r[a].bytes, r[b].p, r[b].bytes)) return true;
  return false;
}

}  // namespace

extern "C" {

int cotr_corr_depth(const float* corr, const uint8_t* valid, const double* cams, const double* poses, int V, int H, int W,
                    const int32_t* found, double threshold, double max_cos, double distance_thresh, int min_views, int refine_iters,
                    float* depth_out, uint8_t* views_out, float* err_out, int32_t* info_out, cotr_stream stream) {
  static const char* fn = "cotr_corr_depth";
  if (V < 2 || V > TV_MAX_VIEWS) return arg_fail(fn, "V must be in [2, 32]");
  if (H < 1 || W < 1 || (long long)H * W > MAX_PIXELS) return arg_fail(fn, "H and W must be >= 1 with at most 2^28 pixels");
  if (!(threshold > 0.0) || !(threshold < INFINITY)) return arg_fail(fn, "threshold must be finite and > 0");
  const float thr = (float)(threshold * threshold);
  if (!(thr > 0.0f) || !(thr < INFINITY)) return arg_fail(fn, "the squared threshold must be a finite float32 that is not 0");
  if (!(max_cos >= -1.0) || !(max_cos <= 1.0)) return arg_fail(fn, "max_cos must be in [-1, 1]");
  if (!(distance_thresh > 0.0) || !(distance_thresh < INFINITY)) return arg_fail(fn, "distance_thresh must be finite and > 0");
  if (min_views < 1 || min_views > TV_MAX_VIEWS - 1) return arg_fail(fn, "min_views must be in [1, 31]");
  if (refine_iters < 0 || refine_iters > MD_MAX_REFINE) return arg_fail(fn, "refine_iters must be in [0, 64]");
  if (!corr || !cams || !poses || !depth_out || !views_out || !err_out || !info_out)
    return arg_fail(fn, "corr, cams, poses, depth_out, views_out, err_out and info_out must not be NULL");
  if (!aligned(corr, 8) || !aligned(cams, 8) || !aligned(poses, 8) || !aligned(depth_out, 4) || !aligned(err_out, 4) ||
      !aligned(info_out, 4) || !aligned(found, 4))
    return arg_fail(fn, "corr and the doubles must be 8-byte, float32 and int32 outputs 4-byte aligned");
  const size_t HW = (size_t)H * W, K = (size_t)(V - 1);
  const MdRange r[] = {{depth_out, HW * 4}, {views_out, HW}, {err_out, HW * 4}, {info_out, 32}, {corr, K * HW * 8}, {valid, K * HW},
                       {cams, (size_t)V * 40}, {poses, (size_t)V * 96}, {found, 4}};
  if (md_alias(r, 9, 4)) return arg_fail(fn, "an output must not overlap another output or an input");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(hl_begin_kernel<>, dim3(1), dim3(64), 0, s, found, 1, 8, info_out);
  hipLaunchKernelGGL(md_depth_kernel, dim3((unsigned)((HW + MD_THREADS - 1) / MD_THREADS)), dim3(MD_THREADS), 0, s, corr, valid, cams, poses, V, H, W,
                     found, thr, max_cos, distance_thresh, min_views, refine_iters, depth_out, views_out, err_out, info_out);
  return launched();
}

int cotr_depth_consistency(const float* depths, int n, int H, int W, const double* Ks, const double* c2w, const int32_t* found,
                           const uint8_t* pairs, double px_thresh, double rel_thresh, int min_views, int max_violations,
                           float* depth_out, uint8_t* count_out, int32_t* info_out, cotr_stream stream) {
  static const char* fn = "cotr_depth_consistency";
  if (n < 2 || n > MD_MAX_MAPS) return arg_fail(fn, "n must be in [2, 32]");
  if (H < 1 || W < 1 || (long long)n * H * W > MAX_PIXELS) return arg_fail(fn, "H and W must be >= 1 with at most 2^28 pixels in all");
  if (!(px_thresh > 0.0) || !md_finite(px_thresh) || !md_finite(px_thresh * px_thresh)) return arg_fail(fn, "px_thresh must be finite and > 0, and so its square");
  if (!(rel_thresh > 0.0) || !(rel_thresh < 1.0)) return arg_fail(fn, "rel_thresh must be in (0, 1)");
  if (min_views < 0 || min_views > MD_MAX_MAPS - 1) return arg_fail(fn, "min_views must be in [0, 31]");
  if (max_violations < -1 || max_violations > MD_MAX_MAPS - 1) return arg_fail(fn, "max_violations must be in [-1, 31]");
  if (!depths || !Ks || !c2w || !depth_out || !count_out || !info_out)
    return arg_fail(fn, "depths, Ks, c2w, depth_out, count_out and info_out must not be NULL");
  EsCams cams;
  if (const char* what = es_cameras(Ks, n, &cams)) return arg_fail(fn, what);
  if (!aligned(depths, 4) || !aligned(c2w, 8) || !aligned(found, 4) || !aligned(depth_out, 4) || !aligned(info_out, 4))
    return arg_fail(fn, "floats and int32 must be 4-byte and doubles 8-byte aligned");
  const size_t HW = (size_t)H * W, all = (size_t)n * HW;
  const MdRange r[] = {{depth_out, all * 4}, {count_out, all}, {info_out, (size_t)n * 16}, {depths, all * 4}, {c2w, (size_t)n * 128},
                       {found, (size_t)n * 4}, {pairs, (size_t)n * n}};
  if (md_alias(r, 7, 3)) return arg_fail(fn, "an output must not overlap another output or an input (depth_out is not depths)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(hl_begin_kernel<>, dim3(1), dim3(64), 0, s, found, n, 4, info_out);
  hipLaunchKernelGGL(md_consistency_kernel, dim3((unsigned)((HW + MD_THREADS - 1) / MD_THREADS), n), dim3(MD_THREADS), 0, s, depths, n, H, W, cams, c2w,
                     found, pairs, px_thresh * px_thresh, rel_thresh, min_views, max_violations, depth_out, count_out, info_out);
  return launched();
}

}  // extern "C"

