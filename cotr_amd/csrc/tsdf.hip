// A truncated signed distance volume of posed depth maps and its raycast (the model half of KinectFusion, whose tracking
// half is icp.hip).  Rules in include/cotr_hip.h and DESIGN.md 3h-11.  tsdf and weight are float32 [Nz][Ny][Nx], x fastest;
// every intermediate is float64.
//
// cotr_tsdf_integrate: 2 launches on the caller's stream, whatever the data:
//   1. ts_begin_kernel          one thread per capture: its info row = {found, 0, 0, 0}
//   2. ts_integrate_kernel      one thread per voxel, consecutive lanes on consecutive x; a workgroup walks TS_ROWS runs of 256
//                               voxels and every thread its captures in order, so the volume is read once and written once
//                               (where a capture updated it) whatever n is.  The counts of a capture: a ballot per wavefront,
//                               one integer add of it into the workgroup's LDS counters, and one integer atomic per
//                               workgroup, capture and counter into info at the end.
// cotr_tsdf_raycast: 2 launches:
//   1. ts_begin_kernel          info = {found, 0, 0, 0}
//   2. ts_raycast_kernel        one thread per pixel, a wavefront on an 8 x 8 pixel tile (a workgroup on 16 x 16), so the 8-corner
//                               gathers of neighbouring rays share cache lines.  Samples outside the volume's box are skipped
//                               without a gather, and a ray that has left the box ends: along a ray the coordinates are
//                               monotone in the sample index (every rounding in s_k = near + k step, p = t + s d and
//                               g = (p - origin) / voxel is monotone), so the samples inside the box are one run of k and every
//                               sample after it is invalid by the rule itself.  The hit and back-face counts: a ballot and one
//                               integer atomic per wavefront.
// Integer atomics only: the same input gives the same bits.  No host waits, no allocation: capturable.  Compiled with
// -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "handleless.h"
#include "pinhole.h"

using namespace cotr_detail;

#define TS_MAX_CAPS 32
#define TS_MAX_VOXELS (1 << 28)
#define TS_MAX_STEPS 65536
#define TS_ROWS 4              // runs of 256 voxels a workgroup of ts_integrate_kernel walks

struct TsGrid {
  int Nx, Ny, Nz;
  double ox, oy, oz, voxel;
};

// the cameras and observation weights of a call: kernel arguments, read at a uniform index
struct TsCaps {
  EsCam k[TS_MAX_CAPS];
  double w[TS_MAX_CAPS];
};

__global__ __launch_bounds__(64) void ts_begin_kernel(const int32_t* __restrict__ found, int n, int32_t* __restrict__ info) {
  const int c = threadIdx.x;
  if (c >= n) return;
  info[c * 4] = found ? (found[c] != 0 ? 1 : 0) : 1;
  info[c * 4 + 1] = info[c * 4 + 2] = info[c * 4 + 3] = 0;
}

// ---- integration ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ts_integrate_kernel(float* __restrict__ tsdf, float* __restrict__ weight, TsGrid g, double trunc,
                                                           const float* __restrict__ depths, int n, int H, int W, TsCaps caps,
                                                           const double* __restrict__ c2w, const int32_t* __restrict__ found,
                                                           double max_weight, int32_t* __restrict__ info) {
  __shared__ int cnt[TS_MAX_CAPS][2];   // voxels updated, voxels whose pixel held a valid depth
  if (threadIdx.x < 2 * TS_MAX_CAPS) (&cnt[0][0])[threadIdx.x] = 0;
  __syncthreads();
  const int total = g.Nx * g.Ny * g.Nz;
  const bool first_lane = (threadIdx.x & 63) == 0;
  for (int r = 0; r < TS_ROWS; ++r) {
    const int idx = (blockIdx.x * TS_ROWS + r) * 256 + threadIdx.x;
    const bool in = idx < total;
    const int row = idx / g.Nx, i = idx - row * g.Nx, k = row / g.Ny, j = row - k * g.Ny;
    const double Px = g.ox + g.voxel * (double)i, Py = g.oy + g.voxel * (double)j, Pz = g.oz + g.voxel * (double)k;
    float T = 0.0f, Wt = 0.0f;
    if (in) T = tsdf[idx], Wt = weight[idx];
    bool touched = false;
    for (int c = 0; c < n; ++c) {
      if (found && found[c] == 0) continue;   // uniform
      const double* __restrict__ m = c2w + c * 16;
      const EsCam& cam = caps.k[c];
      bool valid = false, updated = false;
      if (in) {
        const double dx = Px - m[3], dy = Py - m[7], dz = Pz - m[11];
        const double Yx = (m[0] * dx + m[4] * dy) + m[8] * dz, Yy = (m[1] * dx + m[5] * dy) + m[9] * dz,
                     Yz = (m[2] * dx + m[6] * dy) + m[10] * dz;
        if (Yz > 0.0) {   // false for NaN
          const double xn = Yx / Yz, yn = Yy / Yz;
          const double u = rint((cam.fx * xn + cam.s * yn) + cam.cx), v = rint(cam.fy * yn + cam.cy);
          if (u >= 0.0 && u < (double)W && v >= 0.0 && v < (double)H) {
            const double z = (double)depths[((size_t)c * H + (size_t)(int)v) * W + (size_t)(int)u];
            if (z > 0.0 && z < INFINITY) {
              valid = true;
              const double sdf = z - Yz;
              if (!(sdf < -trunc)) {
                const double d = fmin(1.0, sdf / trunc), w = caps.w[c];
                const double Td = (double)T, Wd = (double)Wt;
                T = (float)((Td * Wd + d * w) / (Wd + w));
                Wt = (float)fmin(Wd + w, max_weight);
                updated = true;
              }
            }
          }
        }
      }
      touched = touched || updated;
      const int nv = __popcll(__ballot(valid)), nu = __popcll(__ballot(updated));
      if (first_lane) {
        if (nu > 0) atomicAdd(&cnt[c][0], nu);
        if (nv > 0) atomicAdd(&cnt[c][1], nv);
      }
    }
    if (touched) tsdf[idx] = T, weight[idx] = Wt;
  }
  __syncthreads();
  if (threadIdx.x < 2 * n) {
    const int v = (&cnt[0][0])[threadIdx.x];
    if (v > 0) atomicAdd(&info[(threadIdx.x >> 1) * 4 + 1 + (threadIdx.x & 1)], v);
  }
}

// ---- the raycast ----------------------------------------------------------------------------------------------------------
struct TsRay {
  EsCam k;
  int H, W, steps;             // samples 0 .. steps
  double near, step;
};

// the grid coordinates of p; false unless floor of each lies in [0, N - 2]
__device__ __forceinline__ bool ts_grid(const TsGrid& g, double px, double py, double pz, double* q) {
  q[0] = (px - g.ox) / g.voxel, q[1] = (py - g.oy) / g.voxel, q[2] = (pz - g.oz) / g.voxel;
  return q[0] >= 0.0 && q[0] < (double)(g.Nx - 1) && q[1] >= 0.0 && q[1] < (double)(g.Ny - 1) && q[2] >= 0.0 && q[2] < (double)(g.Nz - 1);
}

// the trilinear value at grid coordinates inside the box; false unless all 8 corners have been observed
__device__ __forceinline__ bool ts_trilinear(const float* __restrict__ tsdf, const float* __restrict__ weight, const TsGrid& g, const double* q,
                                             double* f) {
  const double bx = floor(q[0]), by = floor(q[1]), bz = floor(q[2]);
  const int b = ((int)bz * g.Ny + (int)by) * g.Nx + (int)bx, sy = g.Nx, sz = g.Nx * g.Ny;
  const float w000 = weight[b], w100 = weight[b + 1], w010 = weight[b + sy], w110 = weight[b + sy + 1];
  const float w001 = weight[b + sz], w101 = weight[b + sz + 1], w011 = weight[b + sz + sy], w111 = weight[b + sz + sy + 1];
  if (!(w000 > 0.0f && w100 > 0.0f && w010 > 0.0f && w110 > 0.0f && w001 > 0.0f && w101 > 0.0f && w011 > 0.0f && w111 > 0.0f)) return false;
  const double a000 = (double)tsdf[b], a100 = (double)tsdf[b + 1], a010 = (double)tsdf[b + sy], a110 = (double)tsdf[b + sy + 1];
  const double a001 = (double)tsdf[b + sz], a101 = (double)tsdf[b + sz + 1], a011 = (double)tsdf[b + sz + sy], a111 = (double)tsdf[b + sz + sy + 1];
  const double rx = q[0] - bx, ry = q[1] - by, rz = q[2] - bz;
  const double c00 = a000 + rx * (a100 - a000), c10 = a010 + rx * (a110 - a010), c01 = a001 + rx * (a101 - a001), c11 = a011 + rx * (a111 - a011);
  const double c0 = c00 + ry * (c10 - c00), c1 = c01 + ry * (c11 - c01);
  *f = c0 + rz * (c1 - c0);
  return true;
}

__device__ __forceinline__ bool ts_sample(const float* __restrict__ tsdf, const float* __restrict__ weight, const TsGrid& g, double px, double py,
                                          double pz, double* f) {
  double q[3];
  return ts_grid(g, px, py, pz, q) && ts_trilinear(tsdf, weight, g, q, f);
}

__global__ __launch_bounds__(256) void ts_raycast_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight, TsGrid g, TsRay ray,
                                                         const double* __restrict__ c2w, const int32_t* __restrict__ found,
                                                         float* __restrict__ depth_out, double* __restrict__ normal_out, int32_t* __restrict__ info) {
  const int tiles_x = (ray.W + 15) >> 4;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int x = tx * 16 + (wave & 1) * 8 + (lane & 7), y = ty * 16 + (wave >> 1) * 8 + (lane >> 3);
  const bool in = x < ray.W && y < ray.H;
  const bool on = found ? found[0] != 0 : true;   // uniform
  int state = 0;               // 1: a hit, 2: ended at a back face
  double s_hit = 0.0, dcz = 0.0, dw[3] = {0.0, 0.0, 0.0};
  if (in && on) {
    const double yn = ((double)y - ray.k.cy) / ray.k.fy;
    const double xn = ((double)x - ray.k.cx - ray.k.s * yn) / ray.k.fx;
    const double norm = sqrt((xn * xn + yn * yn) + 1.0);
    const double dcx = xn / norm, dcy = yn / norm;
    dcz = 1.0 / norm;
#pragma unroll
    for (int a = 0; a < 3; ++a) dw[a] = (c2w[a * 4] * dcx + c2w[a * 4 + 1] * dcy) + c2w[a * 4 + 2] * dcz;
    const double t0 = c2w[3], t1 = c2w[7], t2 = c2w[11];
    bool prev_ok = false, was_in = false;
    double prev_f = 0.0;
    for (int k = 0; k <= ray.steps; ++k) {
      const double s = ray.near + (double)k * ray.step;
      double q[3];
      if (!ts_grid(g, t0 + s * dw[0], t1 + s * dw[1], t2 + s * dw[2], q)) {
        if (was_in) break;     // the samples inside the box are one run of k
        prev_ok = false;
        continue;
      }
      was_in = true;
      double f = 0.0;
      const bool ok = ts_trilinear(tsdf, weight, g, q, &f);
      if (ok && prev_ok) {
        if (prev_f > 0.0 && f <= 0.0) {
          s_hit = (ray.near + (double)(k - 1) * ray.step) + ray.step * (prev_f / (prev_f - f));
          state = 1;
          break;
        }
        if (prev_f < 0.0 && f > 0.0) {
          state = 2;
          break;
        }
      }
      prev_ok = ok, prev_f = f;
    }
  }
  if (in) {
    const size_t p = (size_t)y * ray.W + x;
    depth_out[p] = state == 1 ? (float)(s_hit * dcz) : 0.0f;
    if (normal_out) {
      double nrm[3] = {NAN, NAN, NAN};
      if (!on) nrm[0] = nrm[1] = nrm[2] = 0.0;
      if (state == 1) {
        const double px = c2w[3] + s_hit * dw[0], py = c2w[7] + s_hit * dw[1], pz = c2w[11] + s_hit * dw[2];
        double fp[3], fm[3];
        bool ok = ts_sample(tsdf, weight, g, px + g.voxel, py, pz, &fp[0]) && ts_sample(tsdf, weight, g, px - g.voxel, py, pz, &fm[0]);
        ok = ok && ts_sample(tsdf, weight, g, px, py + g.voxel, pz, &fp[1]) && ts_sample(tsdf, weight, g, px, py - g.voxel, pz, &fm[1]);
        ok = ok && ts_sample(tsdf, weight, g, px, py, pz + g.voxel, &fp[2]) && ts_sample(tsdf, weight, g, px, py, pz - g.voxel, &fm[2]);
        if (ok) {
          const double gx = fp[0] - fm[0], gy = fp[1] - fm[1], gz = fp[2] - fm[2];
          const double len = sqrt((gx * gx + gy * gy) + gz * gz);
          if (len > 0.0) {     // false for NaN
#pragma unroll
            for (int a = 0; a < 3; ++a) nrm[a] = ((c2w[a] * gx + c2w[4 + a] * gy) + c2w[8 + a] * gz) / len;
          }
        }
      }
      normal_out[p * 3] = nrm[0], normal_out[p * 3 + 1] = nrm[1], normal_out[p * 3 + 2] = nrm[2];
    }
  }
  const int nh = __popcll(__ballot(state == 1)), nb = __popcll(__ballot(state == 2));
  if (lane == 0) {
    if (nh > 0) atomicAdd(&info[1], nh);
    if (nb > 0) atomicAdd(&info[2], nb);
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
namespace {

int ts_fail(const char* fn, const char* what) {
  char msg[256];
  snprintf(msg, sizeof msg, "%s: %s", fn, what);
  return handleless_fail(COTR_ERR_ARG, msg);
}

bool ts_finite(double v) { return fabs(v) < INFINITY; }   // false for NaN

// the volume's arguments -> g; the message of the first rule broken, or NULL
const char* ts_check_volume(const float* tsdf, const float* weight, int Nx, int Ny, int Nz, const double* origin, double voxel, TsGrid* g) {
  if (Nx < 2 || Ny < 2 || Nz < 2 || (long long)Nx * Ny * Nz > TS_MAX_VOXELS) return "Nx, Ny and Nz must be >= 2 with at most 2^28 voxels";
  if (!(voxel > 0.0) || !ts_finite(voxel)) return "voxel must be finite and > 0";
  if (!tsdf || !weight || !origin) return "tsdf, weight and origin must not be NULL";
  if (!ts_finite(origin[0]) || !ts_finite(origin[1]) || !ts_finite(origin[2])) return "origin must be finite";
  if (!aligned(tsdf, 4) || !aligned(weight, 4)) return "floats and int32 must be 4-byte and doubles 8-byte aligned";
  *g = {Nx, Ny, Nz, origin[0], origin[1], origin[2], voxel};
  return nullptr;
}

}  // namespace

extern "C" {

int cotr_tsdf_integrate(float* tsdf, float* weight, int Nx, int Ny, int Nz, const double* origin, double voxel, double trunc,
                        const float* depths, int n, int H, int W, const double* Ks, const double* c2w, const int32_t* found,
                        const double* obs_weight, double max_weight, int32_t* info_out, cotr_stream stream) {
  static const char* fn = "cotr_tsdf_integrate";
  TsGrid g;
  if (const char* msg = ts_check_volume(tsdf, weight, Nx, Ny, Nz, origin, voxel, &g)) return ts_fail(fn, msg);
  if (!(trunc > 0.0) || !ts_finite(trunc)) return ts_fail(fn, "trunc must be finite and > 0");
  if (n < 1 || n > TS_MAX_CAPS) return ts_fail(fn, "n must be in [1, 32]");
  if (H < 1 || W < 1 || (long long)H * W > MAX_PIXELS) return ts_fail(fn, "H and W must be >= 1 with at most 2^28 pixels");
  if (!(max_weight > 0.0)) return ts_fail(fn, "max_weight must be > 0");
  if (!depths || !Ks || !c2w || !info_out) return ts_fail(fn, "depths, Ks, c2w and info_out must not be NULL");
  TsCaps caps;
  for (int c = 0; c < TS_MAX_CAPS; ++c) {
    caps.k[c] = {1.0, 1.0, 0.0, 0.0, 0.0};
    caps.w[c] = 1.0;
  }
  for (int c = 0; c < n; ++c) {
    if (!es_camera(Ks + c * 9, &caps.k[c])) return ts_fail(fn, "the camera matrices must be finite with focal lengths that are not 0");
    if (obs_weight) {
      if (!(obs_weight[c] > 0.0) || !ts_finite(obs_weight[c])) return ts_fail(fn, "every obs_weight must be finite and > 0");
      caps.w[c] = obs_weight[c];
    }
  }
  if (!aligned(depths, 4) || !aligned(c2w, 8) || !aligned(found, 4) || !aligned(info_out, 4))
    return ts_fail(fn, "floats and int32 must be 4-byte and doubles 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int total = Nx * Ny * Nz, per_group = 256 * TS_ROWS;
  hipLaunchKernelGGL(ts_begin_kernel, dim3(1), dim3(64), 0, s, found, n, info_out);
  hipLaunchKernelGGL(ts_integrate_kernel, dim3((unsigned)((total + per_group - 1) / per_group)), dim3(256), 0, s, tsdf, weight, g, trunc, depths, n, H,
                     W, caps, c2w, found, max_weight, info_out);
  return launched();
}

int cotr_tsdf_raycast(const float* tsdf, const float* weight, int Nx, int Ny, int Nz, const double* origin, double voxel, const double* K,
                      const double* c2w, const int32_t* found, int H, int W, double near, double far, double step, float* depth_out,
                      double* normal_out, int32_t* info_out, cotr_stream stream) {
  static const char* fn = "cotr_tsdf_raycast";
  TsGrid g;
  if (const char* msg = ts_check_volume(tsdf, weight, Nx, Ny, Nz, origin, voxel, &g)) return ts_fail(fn, msg);
  if (H < 1 || W < 1 || (long long)H * W > MAX_PIXELS) return ts_fail(fn, "H and W must be >= 1 with at most 2^28 pixels");
  if (!(near >= 0.0) || !ts_finite(near)) return ts_fail(fn, "near must be finite and >= 0");
  if (!(far > near) || !ts_finite(far)) return ts_fail(fn, "far must be finite and > near");
  if (!(step > 0.0) || !ts_finite(step)) return ts_fail(fn, "step must be finite and > 0");
  const double steps = ceil((far - near) / step);
  if (!(steps <= (double)TS_MAX_STEPS)) return ts_fail(fn, "ceil((far - near) / step) must be at most 65536");
  if (!K || !c2w || !depth_out || !info_out) return ts_fail(fn, "K, c2w, depth_out and info_out must not be NULL");
  TsRay ray;
  if (!es_camera(K, &ray.k)) return ts_fail(fn, "the camera matrix must be finite with focal lengths that are not 0");
  if (!aligned(c2w, 8) || !aligned(found, 4) || !aligned(depth_out, 4) || !aligned(normal_out, 8) || !aligned(info_out, 4))
    return ts_fail(fn, "floats and int32 must be 4-byte and doubles 8-byte aligned");
  ray.H = H, ray.W = W, ray.steps = (int)steps, ray.near = near, ray.step = step;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned tiles = (unsigned)((W + 15) / 16) * (unsigned)((H + 15) / 16);
  hipLaunchKernelGGL(ts_begin_kernel, dim3(1), dim3(64), 0, s, found, 1, info_out);
  hipLaunchKernelGGL(ts_raycast_kernel, dim3(tiles), dim3(256), 0, s, tsdf, weight, g, ray, c2w, found, depth_out, normal_out, info_out);
  return launched();
}

}  // extern "C"
