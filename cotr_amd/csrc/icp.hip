// Dense refinement of the rigid motion between two depth maps: projective data association with a point-to-plane
// Gauss-Newton step (the ICP of KinectFusion).  Rules in DESIGN.md 3h-9.  x_a = R x_b + t.
//
// cotr_icp_depth: 3 + 2 * (iters + 1) launches on the caller's stream, whatever the data:
//   1. ic_begin_kernel          one thread: the start pose into the state (through the rigid inverse of c2w_a when given),
//                               the counters zeroed, the `found` gate
//   2. ic_map_kernel            twice, once per capture, one thread per pixel: the vertex of the pixel centre and the normal
//                               from the central differences of the four neighbours' vertices -> scratch as float64 (NaN
//                               where there is none); B's launch also writes the mask of the source pixels and counts them
//   3. iters + 1 pairs of rf_accum_kernel<IcTerms> (per 2048-pixel chunk of the source pixels in row-major order: 29 sums,
//      every thread over its pixels in order, every wavefront in a fixed butterfly, the 4 wavefronts in order -> scratch)
//      and ic_finish_kernel (one workgroup: the chunks in chunk order, then one thread: stop, or the eigen-decomposition of
//      the normal matrix by rs_jacobi<6> and the step).  refit.h's frame with its accumulate and reduce as they are; the
//      finish is the file's own, because the pairs change with the pose: there is no fixed objective whose fall could be
//      asked for, so every solvable step is taken.  The last pair only evaluates, and writes the outputs (back through
//      c2w_a when given).  A device-side flag idles the chain after a stop; its length never depends on the data.
// Integer atomics only (the two counts of valid normals): the same input gives the same bits.  No host waits, no
// allocation: capturable.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "handleless.h"
#include "icp_maps.h"
#include "ransac.h"
#include "refit.h"

using namespace cotr_detail;

#define IC_SUMS 29             // 21 of J^T J, 6 of J^T r, the squared error, the pairs
#define IC_HIST 32             // a row of hist_out: the sums, l_min, l_max, 0
#define IC_MIN_PAIRS 6
#define IC_MAX_ITERS 64
#define IC_MAX_STRIDE 64

// the state of the chain, in scratch, and the pose of refit.h: exp([w]x) R, t + dt
struct IcState : RfPose {
  static constexpr int PARAMS = 6;
  double Ra[9], ta[3];         // c2w_a, when given
  double err;                  // sum r^2 of the last evaluation
  int has_c2w, found;
  int pairs, reason;           // of the last evaluation; the stop reason
  int valid[2];                // pixels with a valid normal: A's, B's source pixels
};

// what one source pixel is paired through
struct IcPoints {
  const double* __restrict__ Va;
  const double* __restrict__ Na;
  const double* __restrict__ Vb;
  const double* __restrict__ Nb;
  int32_t* __restrict__ assoc;
  EsCam ka;
  int Ha, Wa, Wb, stride, ws;  // ws: source pixels in a row
  double max_d2, normal_cos;
};

// ---- the maps (the pixel rule: icp_maps.h) --------------------------------------------------------------------------------
// One thread per pixel -> V[H W][3], N[H W][3] (NaN where invalid; the same to maps_out[H W][6] when given), the count of
// valid normals.  which = 1 (B): only the source pixels are counted, those with x % stride == 0 and y % stride == 0 that
// src_mask admits; source pixel j gets smask[j] = counted and assoc[j] = -1.
__global__ __launch_bounds__(256) void ic_map_kernel(const float* __restrict__ depth, int H, int W, EsCam k, double edge, int which, int stride,
                                                     int ws, const uint8_t* __restrict__ src_mask, double* __restrict__ V, double* __restrict__ N,
                                                     double* __restrict__ maps_out, uint8_t* __restrict__ smask, int32_t* __restrict__ assoc,
                                                     IcState* __restrict__ st) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  const bool in = p < H * W;
  bool counted = false;
  if (in) {
    const int y = p / W, x = p - y * W;
    double v[3], n[3];
    const bool ok = ic_pixel(depth, H, W, k, edge, x, y, v, n);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      V[(size_t)p * 3 + c] = v[c];
      N[(size_t)p * 3 + c] = n[c];
      if (maps_out) maps_out[(size_t)p * 6 + c] = v[c], maps_out[(size_t)p * 6 + 3 + c] = n[c];
    }
    counted = ok;
    if (which == 1) {
      const bool source = x % stride == 0 && y % stride == 0;
      counted = source && ok && (!src_mask || src_mask[p] != 0);
      if (source) {
        const int j = (y / stride) * ws + x / stride;
        smask[j] = counted ? 1 : 0;
        if (assoc) assoc[j] = -1;
      }
    }
  }
  const int wc = __popcll(__ballot(counted));
  if ((threadIdx.x & 63) == 0 && wc > 0) atomicAdd(&st->valid[which], wc);
}

// ---- one evaluation -------------------------------------------------------------------------------------------------------
// One source pixel's terms at the pose of st, added to acc: J^T J (21), J^T r (6), r^2 and 1, when it passes every gate; its
// pixel of A, or -1, to assoc.  The residual is n_a . (Y - V_a) with Y = R X_b + t; over (w, dt) of exp([w]x) R, t + dt its
// Jacobian row is ((R X_b) x n_a, n_a).
struct IcTerms {
  static constexpr int SUMS = IC_SUMS, STRIDE = IC_SUMS;
  using Points = IcPoints;
  using State = IcState;
  static __device__ __forceinline__ void terms(const IcState* __restrict__ st, const IcPoints& pts, int p, double* acc) {
    const int sy = p / pts.ws, sx = p - sy * pts.ws;
    const size_t b = (size_t)(sy * pts.stride) * pts.Wb + sx * pts.stride;
    const double* R = st->R;
    const double X[3] = {pts.Vb[b * 3], pts.Vb[b * 3 + 1], pts.Vb[b * 3 + 2]};
    const double Px = (R[0] * X[0] + R[1] * X[1]) + R[2] * X[2], Py = (R[3] * X[0] + R[4] * X[1]) + R[5] * X[2],
                 Pz = (R[6] * X[0] + R[7] * X[1]) + R[8] * X[2];
    const double Y[3] = {Px + st->t[0], Py + st->t[1], Pz + st->t[2]};
    double u, v;
    int a = -1, ax, ay;
    if (es_project(pts.ka, Y, &u, &v) && es_nearest(u, v, pts.Ha, pts.Wa, &ax, &ay)) {   // pinhole.h: Y_z > 0, a pixel of A
      const size_t q = (size_t)ay * pts.Wa + ax;
      const double nx = pts.Na[q * 3], ny = pts.Na[q * 3 + 1], nz = pts.Na[q * 3 + 2];
      if (nx == nx) {   // A has a valid normal there
        const double dx = Y[0] - pts.Va[q * 3], dy = Y[1] - pts.Va[q * 3 + 1], dz = Y[2] - pts.Va[q * 3 + 2];
        if ((dx * dx + dy * dy) + dz * dz <= pts.max_d2) {
          const double mx = pts.Nb[b * 3], my = pts.Nb[b * 3 + 1], mz = pts.Nb[b * 3 + 2];
          const double Rx = (R[0] * mx + R[1] * my) + R[2] * mz, Ry = (R[3] * mx + R[4] * my) + R[5] * mz,
                       Rz = (R[6] * mx + R[7] * my) + R[8] * mz;
          if ((Rx * nx + Ry * ny) + Rz * nz >= pts.normal_cos) {
            a = (int)q;
            const double r = (nx * dx + ny * dy) + nz * dz;
            const double J[6] = {Py * nz - Pz * ny, Pz * nx - Px * nz, Px * ny - Py * nx, nx, ny, nz};
#pragma unroll
            for (int i = 0; i < 6; ++i) {
#pragma unroll
              for (int j = i; j < 6; ++j) acc[rf_tri<6>(i, j)] += J[i] * J[j];
              acc[21 + i] += J[i] * r;
            }
            acc[27] += r * r;
            acc[28] += 1.0;
          }
        }
      }
    }
    if (pts.assoc) pts.assoc[p] = a;
  }
};

// ---- the chain ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void ic_begin_kernel(const double* __restrict__ R0, const double* __restrict__ t0, const double* __restrict__ c2w_a,
                                                      const int32_t* __restrict__ found, IcState* __restrict__ st) {
  if (threadIdx.x != 0) return;
  const int f = found ? (found[0] != 0) : 1;
  double R[9], t[3];
  for (int i = 0; i < 9; ++i) R[i] = R0[i];
  for (int i = 0; i < 3; ++i) t[i] = t0[i];
  st->has_c2w = c2w_a ? 1 : 0;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) st->Ra[i * 3 + j] = c2w_a ? c2w_a[i * 4 + j] : 0.0;
    st->ta[i] = c2w_a ? c2w_a[i * 4 + 3] : 0.0;
  }
  if (c2w_a) {   // the rigid inverse: R_a^T, -R_a^T t_a
    const double* A = st->Ra;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) st->R[i * 3 + j] = (A[i] * R[j] + A[3 + i] * R[3 + j]) + A[6 + i] * R[6 + j];
      const double ti = -((A[i] * st->ta[0] + A[3 + i] * st->ta[1]) + A[6 + i] * st->ta[2]);
      st->t[i] = ((A[i] * t[0] + A[3 + i] * t[1]) + A[6 + i] * t[2]) + ti;
    }
  } else {
    for (int i = 0; i < 9; ++i) st->R[i] = R[i];
    for (int i = 0; i < 3; ++i) st->t[i] = t[i];
  }
  RfPose::save(st);
  st->err_prev = 0.0, st->err = 0.0;
  st->done = f ? 0 : 1;
  st->kept = 0, st->trial = 0;
  st->found = f;
  st->pairs = 0, st->reason = 0;
  st->valid[0] = st->valid[1] = 0;
}

// The sums of evaluation k: stop (fewer than 6 pairs, a sum that is not finite, l_min <= cond_tol l_max of the normal
// matrix), or take the step -V diag(1 / l) V^T (J^T r); the last one only evaluates and writes the outputs.
__global__ __launch_bounds__(64) void ic_finish_kernel(int chunks, const double* __restrict__ parts, IcState* __restrict__ st, int k, int last,
                                                       double cond_tol, double* __restrict__ R_out, double* __restrict__ t_out,
                                                       int32_t* __restrict__ info, double* __restrict__ stats, double* __restrict__ hist) {
  __shared__ double sums[IC_HIST];
  const bool active = !st->done;   // uniform; read before anything below writes it
  rf_reduce<IC_SUMS>(parts, chunks, active ? IC_SUMS : 0, sums);
  if (threadIdx.x != 0) return;
  double lmin = 0.0, lmax = 0.0;
  if (active) {
    const int pairs = (int)sums[28];
    st->pairs = pairs;
    st->err = sums[27];
    bool finite = true;
    for (int i = 0; i < 28; ++i) finite = finite && fabs(sums[i]) < INFINITY;   // false for NaN
    int reason = 0;
    if (pairs < IC_MIN_PAIRS) {
      reason = 1;
    } else if (!finite) {
      reason = 3;
    } else if (!last) {
      double a[6][6], v[6][6];
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) a[i][j] = a[j][i] = sums[rf_tri<6>(i, j)];
      rs_jacobi<6>(a, v);
      lmin = lmax = a[0][0];
#pragma unroll
      for (int i = 1; i < 6; ++i) {
        if (a[i][i] < lmin) lmin = a[i][i];
        if (a[i][i] > lmax) lmax = a[i][i];
      }
      if (!(lmin > cond_tol * lmax)) {   // also for NaN
        reason = 2;
      } else {
        double c[6], d[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          double s = 0.0;
#pragma unroll
          for (int i = 0; i < 6; ++i) s += v[i][j] * sums[21 + i];
          c[j] = s / a[j][j];
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          double s = 0.0;
#pragma unroll
          for (int j = 0; j < 6; ++j) s += v[i][j] * c[j];
          d[i] = -s;
        }
        RfPose::rotate(st, d);
        for (int i = 0; i < 3; ++i) st->t[i] = st->t[i] + d[3 + i];
        st->kept = st->kept + 1;
      }
    }
    st->reason = reason;
    if (reason != 0 || last) st->done = 1;
  }
  if (hist) {
    for (int i = 0; i < IC_HIST; ++i) {
      double h = 0.0;
      if (active) h = i < IC_SUMS ? sums[i] : (i == IC_SUMS ? lmin : (i == IC_SUMS + 1 ? lmax : 0.0));
      hist[(size_t)k * IC_HIST + i] = h;
    }
  }
  if (!last) return;
  const int found = st->found;
  const double* R = st->R;
  const double* t = st->t;
  if (st->has_c2w) {
    const double* A = st->Ra;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) R_out[i * 3 + j] = found ? (A[i * 3] * R[j] + A[i * 3 + 1] * R[3 + j]) + A[i * 3 + 2] * R[6 + j] : 0.0;
      t_out[i] = found ? ((A[i * 3] * t[0] + A[i * 3 + 1] * t[1]) + A[i * 3 + 2] * t[2]) + st->ta[i] : 0.0;
    }
  } else {
    for (int i = 0; i < 9; ++i) R_out[i] = found ? R[i] : 0.0;
    for (int i = 0; i < 3; ++i) t_out[i] = found ? t[i] : 0.0;
  }
  const int pairs = found ? st->pairs : 0;
  const double err = found ? st->err : 0.0;
  info[0] = found && st->reason == 0 ? 1 : 0;
  info[1] = found ? st->kept : 0;
  info[2] = pairs;
  info[3] = found ? st->reason : 0;
  info[4] = found ? st->valid[1] : 0;
  info[5] = found ? st->valid[0] : 0;
  info[6] = 0;
  info[7] = 0;
  stats[0] = err;
  stats[1] = pairs > 0 ? sqrt(err / (double)pairs) : 0.0;
}

// ---- host side ------------------------------------------------------------------------------------------------------------
namespace {

int ic_fail(const char* what) { return arg_fail("cotr_icp_depth", what); }

// the state, the per-chunk sums [chunks, IC_SUMS], A's vertices and normals [Ha Wa, 3] each, B's, the source mask [n_src]
struct IcPlan {
  RfPlan rf;
  double *va, *na, *vb, *nb;
  uint8_t* smask;
  size_t bytes;
  int ws, hs, n_src;
};

IcPlan ic_plan(void* base, int Ha, int Wa, int Hb, int Wb, int stride) {
  IcPlan l;
  l.ws = (Wb + stride - 1) / stride;
  l.hs = (Hb + stride - 1) / stride;
  l.n_src = l.ws * l.hs;
  l.rf = rf_plan(0, sizeof(IcState), l.n_src, IC_SUMS);
  const size_t a = (size_t)Ha * Wa * 3, b = (size_t)Hb * Wb * 3;
  Carver c(base, l.rf.bytes);
  l.va = c.take<double>(a);
  l.na = c.take<double>(a);
  l.vb = c.take<double>(b);
  l.nb = c.take<double>(b);
  l.smask = c.take<uint8_t>(l.n_src);
  l.bytes = c.bytes;
  return l;
}

int ic_check_shape(int Ha, int Wa, int Hb, int Wb, int stride) {
  if (Ha < 3 || Wa < 3 || Hb < 3 || Wb < 3 || (long long)Ha * Wa > MAX_PIXELS || (long long)Hb * Wb > MAX_PIXELS)
    return ic_fail("H and W must be >= 3 with at most 2^28 pixels on both sides");
  if (stride < 1 || stride > IC_MAX_STRIDE) return ic_fail("stride must be in [1, 64]");
  return COTR_OK;
}

}  // namespace

extern "C" {

int cotr_icp_depth_scratch_bytes(int Ha, int Wa, int Hb, int Wb, int stride, size_t* bytes) {
  if (const int rc = ic_check_shape(Ha, Wa, Hb, Wb, stride)) return rc;
  if (!bytes) return ic_fail("bytes must not be NULL");
  *bytes = ic_plan(nullptr, Ha, Wa, Hb, Wb, stride).bytes;
  return COTR_OK;
}

int cotr_icp_depth(const float* depth_a, int Ha, int Wa, const double* K_a, const float* depth_b, int Hb, int Wb, const double* K_b,
                   const double* R0, const double* t0, const double* c2w_a, const int32_t* found, const uint8_t* src_mask, double max_dist,
                   double normal_cos, double edge, double cond_tol, int iters, int stride, double* R_out, double* t_out, int32_t* info_out,
                   double* stats_out, double* hist_out, int32_t* assoc_out, double* maps_a_out, double* maps_b_out, void* scratch,
                   size_t scratch_bytes, cotr_stream stream) {
  if (const int rc = ic_check_shape(Ha, Wa, Hb, Wb, stride)) return rc;
  if (iters < 0 || iters > IC_MAX_ITERS) return ic_fail("iters must be in [0, 64]");
  if (!(max_dist > 0.0) || !(max_dist < INFINITY)) return ic_fail("max_dist must be finite and > 0");
  if (!(normal_cos >= -1.0) || !(normal_cos <= 1.0)) return ic_fail("normal_cos must be in [-1, 1]");
  if (!(edge > 0.0) || !(edge < INFINITY)) return ic_fail("edge must be finite and > 0");
  if (!(cond_tol > 0.0) || !(cond_tol < 1.0)) return ic_fail("cond_tol must be in (0, 1)");
  if (!depth_a || !depth_b || !K_a || !K_b || !R0 || !t0 || !R_out || !t_out || !info_out || !stats_out || !scratch)
    return ic_fail("depth_a, depth_b, K_a, K_b, R0, t0, R_out, t_out, info_out, stats_out and scratch must not be NULL");
  EsCam ka, kb;
  if (!es_camera(K_a, &ka) || !es_camera(K_b, &kb)) return ic_fail(ES_CAMERAS_WHAT);
  if (!aligned(depth_a, 4) || !aligned(depth_b, 4) || !aligned(R0, 8) || !aligned(t0, 8) || !aligned(c2w_a, 8) || !aligned(found, 4) ||
      !aligned(R_out, 8) || !aligned(t_out, 8) || !aligned(info_out, 4) || !aligned(stats_out, 8) || !aligned(hist_out, 8) ||
      !aligned(assoc_out, 4) || !aligned(maps_a_out, 8) || !aligned(maps_b_out, 8) || !aligned(scratch, 16))
    return ic_fail("floats and int32 must be 4-byte, doubles 8-byte and scratch 16-byte aligned");
  const IcPlan l = ic_plan(scratch, Ha, Wa, Hb, Wb, stride);
  if (scratch_bytes < l.bytes) return ic_fail("scratch is smaller than cotr_icp_depth_scratch_bytes asks for");
  IcState* st = reinterpret_cast<IcState*>(static_cast<char*>(scratch) + l.rf.state);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(ic_begin_kernel, dim3(1), dim3(64), 0, s, R0, t0, c2w_a, found, st);
  hipLaunchKernelGGL(ic_map_kernel, dim3((unsigned)((Ha * Wa + 255) / 256)), dim3(256), 0, s, depth_a, Ha, Wa, ka, edge, 0, 1, Wa,
                     (const uint8_t*)nullptr, l.va, l.na, maps_a_out, (uint8_t*)nullptr, (int32_t*)nullptr, st);
  hipLaunchKernelGGL(ic_map_kernel, dim3((unsigned)((Hb * Wb + 255) / 256)), dim3(256), 0, s, depth_b, Hb, Wb, kb, edge, 1, stride, l.ws,
                     src_mask, l.vb, l.nb, maps_b_out, l.smask, assoc_out, st);
  const IcPoints pts = {l.va, l.na, l.vb, l.nb, assoc_out, ka, Ha, Wa, Wb, stride, l.ws, max_dist * max_dist, normal_cos};
  for (int k = 0; k <= iters; ++k)
    rf_enqueue_pair<IcTerms>(s, l.rf, scratch, pts, l.n_src, l.smask, ic_finish_kernel, k, (int)(k == iters), cond_tol, R_out, t_out, info_out,
                             stats_out, hist_out);
  return launched();
}

}  // extern "C"
