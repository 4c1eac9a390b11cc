// A truncated signed distance volume of posed depth maps and its raycast (the model half of KinectFusion, whose tracking
// half is icp.hip).  Rules in include/cotr_hip.h and DESIGN.md 3h-11.  tsdf and weight are float32 [Nz][Ny][Nx], x fastest;
// every intermediate is float64.
//
// cotr_tsdf_integrate: 2 launches on the caller's stream, whatever the data:
//   1. hl_begin_kernel          (handleless.h) one thread per capture: its info row = {found, 0, 0, 0}
//   2. ts_integrate_kernel      one thread per voxel, consecutive lanes on consecutive x; a workgroup walks TS_ROWS runs of 256
//                               voxels and every thread its captures in order, so the volume is read once and written once
//                               (where a capture updated it) whatever n is.  The counts of a capture: a ballot per wavefront,
//                               one integer add of it into the workgroup's LDS counters, and one integer atomic per
//                               workgroup, capture and counter into info at the end.
// cotr_tsdf_raycast: 2 launches:
//   1. hl_begin_kernel          info = {found, 0, 0, 0}
//   2. ts_raycast_kernel        one thread per pixel, a wavefront on an 8 x 8 pixel tile (a workgroup on 16 x 16), so the 8-corner
//                               gathers of neighbouring rays share cache lines.  Samples outside the volume's box are skipped
//                               without a gather, and a ray that has left the box ends: along a ray the coordinates are
//                               monotone in the sample index (every rounding in s_k = near + k step, p = t + s d and
//                               g = (p - origin) / voxel is monotone), so the samples inside the box are one run of k and every
//                               sample after it is invalid by the rule itself.  The hit and back-face counts: a ballot and one
//                               integer atomic per wavefront.
// cotr_tsdf_mesh (marching tetrahedra on the Kuhn split of every cell): 4 launches to count, 1 or 2 more to write:
//   1. hl_begin_kernel          info = {found, 0, 0, 0}
//   2. ms_classify_kernel       one thread per voxel: the cell above it is valid, and the inside bits of its 8 corners (2 B a voxel
//                               of scratch).  A lane reads its column of 4 voxels and takes the column at x + 1 from the next lane.
//   3. ms_count_kernel          one thread per voxel, blocks of 512 voxels: the 7 live bits of the voxel's edges from the codes of the
//                               (at most 4) cells that hold each, the triangles of its cell, and both counts (packed in one int) summed
//                               inside the block by scan.h -> a 4 B record a voxel (written only
//                               where the block holds a vertex) and the block's two totals.  Valid cells: ballots summed in a register
//                               of each wavefront, four LDS slots, one integer atomic per workgroup into info.  2 and 3 run on at most
//                               2048 workgroups that walk the blocks: one walk covers 2048 * 512 = 2^20 voxels.
//   4. ms_scan_kernel           one workgroup of 1024: the block totals summed by scan.h, both carried together; the counts.
//   5. ms_emit_kernel           (a capacity above 0) a workgroup whose block has neither vertex nor triangle leaves; a thread writes
//                               the vertices (and normals) of its voxel's live edges and the triangles of its cell: a vertex index
//                               is the scanned base of the edge's voxel + the live bits below the edge's code.
//   6. ms_pad_kernel            (cap_tris above 0) -1 into the triangle rows past the count.
// Every position comes from the scan, none from an atomic.
// The colour volume, float32 [Nz][Ny][Nx][4] = (r, g, b, colour weight), 2 launches each:
//   cotr_tsdf_color_integrate   hl_begin_kernel, then ts_color_integrate_kernel: ts_integrate_kernel's mapping and counters, a voxel
//                               one 16-byte load and, where a capture coloured it, one 16-byte store.
//   cotr_tsdf_color_points      hl_begin_kernel, then ts_color_points_kernel: one thread per point (no second launch without points).
//   cotr_tsdf_color_map         hl_begin_kernel, then ts_color_map_kernel: one thread per pixel on the raycast's tiles.
//                               Both blend the coloured corners of the point's cell through ts_color_at.
// The camera and pose arithmetic is pinhole.h's.  Integer atomics only: the same input gives the same bits.  No host waits, no
// allocation: capturable.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "handleless.h"
#include "pinhole.h"
#include "scan.h"

using namespace cotr_detail;

#define TS_MAX_CAPS ES_MAX_CAMS
#define TS_MAX_VOXELS (1 << 28)
#define TS_MAX_STEPS 65536
#define TS_MAX_POINTS (1 << 28)
#define TS_ROWS 4              // runs of 256 voxels a workgroup of ts_integrate_kernel walks

struct TsGrid {
  int Nx, Ny, Nz;
  double ox, oy, oz, voxel;
};

// the cameras and observation weights of a call: kernel arguments, read at a uniform index
struct TsCaps {
  EsCams cams;
  double w[TS_MAX_CAPS];
};

// ---- integration ----------------------------------------------------------------------------------------------------------
// The voxel centre P seen by capture c (pose m, camera cam): false unless Y_z > 0, the pixel (rint u, rint v) of its projection
// lies inside the map and the depth z there is finite and > 0; then *pix is that pixel's index in depths ([n][H][W]) and
// *sdf = z - Y_z.  Both integrate kernels call it; the arithmetic is pinhole.h's.
__device__ __forceinline__ bool ts_project(const double* __restrict__ m, const EsCam& cam, const double* P, const float* __restrict__ depths, int c,
                                           int H, int W, size_t* pix, double* sdf) {
  double Y[3], u, v;
  es_to_camera(m, P, Y);
  int x, y;
  if (!es_project(cam, Y, &u, &v) || !es_nearest(u, v, H, W, &x, &y)) return false;
  *pix = (size_t)c * H * W + (size_t)(y * W + x);
  const double z = (double)depths[*pix];
  if (!(z > 0.0 && z < INFINITY)) return false;
  *sdf = z - Y[2];
  return true;
}

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
    const double P[3] = {g.ox + g.voxel * (double)i, g.oy + g.voxel * (double)j, g.oz + g.voxel * (double)k};
    float T = 0.0f, Wt = 0.0f;
    if (in) T = tsdf[idx], Wt = weight[idx];
    bool touched = false;
    for (int c = 0; c < n; ++c) {
      if (found && found[c] == 0) continue;   // uniform
      bool valid = false, updated = false;
      size_t pix;
      double sdf;
      if (in && ts_project(c2w + c * 16, caps.cams.k[c], P, depths, c, H, W, &pix, &sdf)) {
        valid = true;
        if (!(sdf < -trunc)) {
          const double d = fmin(1.0, sdf / trunc), w = caps.w[c];
          const double Td = (double)T, Wd = (double)Wt;
          T = (float)((Td * Wd + d * w) / (Wd + w));
          Wt = (float)fmin(Wd + w, max_weight);
          updated = true;
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

// The colour volume: ts_integrate_kernel's mapping and counters on float4 voxels (r, g, b, colour weight).  A
// voxel is one 16-byte load, and one 16-byte store only where a capture coloured it: where its pixel holds a valid depth and
// sdf lies in [-trunc, trunc].  tsdf and weight are not read.
__global__ __launch_bounds__(256) void ts_color_integrate_kernel(float4* __restrict__ color, TsGrid g, double trunc, const float* __restrict__ depths,
                                                                 const uint8_t* __restrict__ images, int n, int H, int W, TsCaps caps,
                                                                 const double* __restrict__ c2w, const int32_t* __restrict__ found,
                                                                 double max_weight, int32_t* __restrict__ info) {
  __shared__ int cnt[TS_MAX_CAPS][2];   // voxels coloured, voxels whose pixel held a valid depth
  if (threadIdx.x < 2 * TS_MAX_CAPS) (&cnt[0][0])[threadIdx.x] = 0;
  __syncthreads();
  const int total = g.Nx * g.Ny * g.Nz;
  const bool first_lane = (threadIdx.x & 63) == 0;
  for (int r = 0; r < TS_ROWS; ++r) {
    const int idx = (blockIdx.x * TS_ROWS + r) * 256 + threadIdx.x;
    const bool in = idx < total;
    const int row = idx / g.Nx, i = idx - row * g.Nx, k = row / g.Ny, j = row - k * g.Ny;
    const double P[3] = {g.ox + g.voxel * (double)i, g.oy + g.voxel * (double)j, g.oz + g.voxel * (double)k};
    float4 C = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (in) C = color[idx];
    bool touched = false;
    for (int c = 0; c < n; ++c) {
      if (found && found[c] == 0) continue;   // uniform
      bool valid = false, coloured = false;
      size_t pix;
      double sdf;
      if (in && ts_project(c2w + c * 16, caps.cams.k[c], P, depths, c, H, W, &pix, &sdf)) {
        valid = true;
        if (!(sdf < -trunc) && !(sdf > trunc)) {
          const uint8_t* __restrict__ p = images + pix * 3;
          const double w = caps.w[c], Wd = (double)C.w, sum = Wd + w;
          C.x = (float)(((double)C.x * Wd + (double)p[0] * w) / sum);
          C.y = (float)(((double)C.y * Wd + (double)p[1] * w) / sum);
          C.z = (float)(((double)C.z * Wd + (double)p[2] * w) / sum);
          C.w = (float)fmin(sum, max_weight);
          coloured = true;
        }
      }
      touched = touched || coloured;
      const int nv = __popcll(__ballot(valid)), nc = __popcll(__ballot(coloured));
      if (first_lane) {
        if (nc > 0) atomicAdd(&cnt[c][0], nc);
        if (nv > 0) atomicAdd(&cnt[c][1], nv);
      }
    }
    if (touched) color[idx] = C;
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

// the validity of a sample at grid coordinates q, before its corners are looked at: floor of each lies in [0, N - 2]
__device__ __forceinline__ bool ts_in_box(const TsGrid& g, const double* q) {
  return q[0] >= 0.0 && q[0] < (double)(g.Nx - 1) && q[1] >= 0.0 && q[1] < (double)(g.Ny - 1) && q[2] >= 0.0 && q[2] < (double)(g.Nz - 1);
}

// the grid coordinates of p; false unless they lie in the box
__device__ __forceinline__ bool ts_grid(const TsGrid& g, double px, double py, double pz, double* q) {
  q[0] = (px - g.ox) / g.voxel, q[1] = (py - g.oy) / g.voxel, q[2] = (pz - g.oz) / g.voxel;
  return ts_in_box(g, q);
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
    double xn, yn;
    es_ray(ray.k, (double)x, (double)y, &xn, &yn);
    const double norm = sqrt((xn * xn + yn * yn) + 1.0);
    dcz = 1.0 / norm;
    const double dc[3] = {xn / norm, yn / norm, dcz};
    es_rotate(c2w, dc, dw);
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
          const double gr[3] = {fp[0] - fm[0], fp[1] - fm[1], fp[2] - fm[2]};
          const double len = sqrt((gr[0] * gr[0] + gr[1] * gr[1]) + gr[2] * gr[2]);
          if (len > 0.0) {     // false for NaN
            es_unrotate(c2w, gr, nrm);
            nrm[0] = nrm[0] / len, nrm[1] = nrm[1] / len, nrm[2] = nrm[2] / len;
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

// ---- the colour of points and of a depth map ---------------------------------------------------------------
// The colour of the world point p as three bytes in bits 0-7, 8-15 and 16-23, and bit 24 set; 0 unless p lies in the box (faces
// included, wider than ts_in_box: a mesh vertex on the last voxel layer has a colour) and a corner of its cell is coloured.  The
// blend is renormalised over the coloured corners, walked with dx fastest, then dy, then dz.
__device__ __forceinline__ unsigned ts_color_at(const float4* __restrict__ color, const TsGrid& g, double px, double py, double pz) {
  const double qx = (px - g.ox) / g.voxel, qy = (py - g.oy) / g.voxel, qz = (pz - g.oz) / g.voxel;
  if (!(qx >= 0.0 && qx <= (double)(g.Nx - 1) && qy >= 0.0 && qy <= (double)(g.Ny - 1) && qz >= 0.0 && qz <= (double)(g.Nz - 1))) return 0u;   // NaN too
  const double bx = fmin(floor(qx), (double)(g.Nx - 2)), by = fmin(floor(qy), (double)(g.Ny - 2)), bz = fmin(floor(qz), (double)(g.Nz - 2));
  const double rx = qx - bx, ry = qy - by, rz = qz - bz;
  const int b = ((int)bz * g.Ny + (int)by) * g.Nx + (int)bx, sy = g.Nx, sz = g.Nx * g.Ny;
  double S = 0.0, Cr = 0.0, Cg = 0.0, Cb = 0.0;
#pragma unroll
  for (int d = 0; d < 8; ++d) {
    const double beta = (((d & 1) ? rx : 1.0 - rx) * ((d & 2) ? ry : 1.0 - ry)) * ((d & 4) ? rz : 1.0 - rz);
    const float4 c = color[b + (d & 1) + ((d >> 1) & 1) * sy + (d >> 2) * sz];
    if (c.w > 0.0f) S += beta, Cr += beta * (double)c.x, Cg += beta * (double)c.y, Cb += beta * (double)c.z;
  }
  if (!(S > 0.0)) return 0u;
  const double r8 = fmin(fmax(rint(Cr / S), 0.0), 255.0), g8 = fmin(fmax(rint(Cg / S), 0.0), 255.0), b8 = fmin(fmax(rint(Cb / S), 0.0), 255.0);
  return (unsigned)r8 | (unsigned)g8 << 8 | (unsigned)b8 << 16 | 1u << 24;
}

__global__ __launch_bounds__(256) void ts_color_points_kernel(const float4* __restrict__ color, TsGrid g, const double* __restrict__ points, int n,
                                                              const int32_t* __restrict__ found, uint8_t* __restrict__ rgb_out,
                                                              uint8_t* __restrict__ valid_out, int32_t* __restrict__ info) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  const bool on = found ? found[0] != 0 : true;   // uniform
  unsigned c = 0u;
  if (p < n && on) c = ts_color_at(color, g, points[(size_t)p * 3], points[(size_t)p * 3 + 1], points[(size_t)p * 3 + 2]);
  if (p < n) {
    rgb_out[(size_t)p * 3] = (uint8_t)(c & 255u), rgb_out[(size_t)p * 3 + 1] = (uint8_t)((c >> 8) & 255u), rgb_out[(size_t)p * 3 + 2] = (uint8_t)((c >> 16) & 255u);
    valid_out[p] = (uint8_t)(c >> 24);
  }
  const int nv = __popcll(__ballot((c >> 24) != 0u));
  if ((threadIdx.x & 63) == 0 && nv > 0) atomicAdd(&info[1], nv);
}

// pixels tiled as in ts_raycast_kernel: the 8-corner gathers of neighbouring pixels share lines
__global__ __launch_bounds__(256) void ts_color_map_kernel(const float4* __restrict__ color, TsGrid g, const float* __restrict__ depth, EsCam cam, int H,
                                                           int W, const double* __restrict__ c2w, const int32_t* __restrict__ found,
                                                           uint8_t* __restrict__ rgb_out, int32_t* __restrict__ info) {
  const int tiles_x = (W + 15) >> 4;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int x = tx * 16 + (wave & 1) * 8 + (lane & 7), y = ty * 16 + (wave >> 1) * 8 + (lane >> 3);
  const bool in = x < W && y < H;
  const bool on = found ? found[0] != 0 : true;   // uniform
  unsigned c = 0u;
  bool has = false;
  if (in && on) {
    double Y[3], P[3];
    has = es_vertex(depth, W, cam, x, y, Y);
    if (has) {
      es_to_world(c2w, Y, P);
      c = ts_color_at(color, g, P[0], P[1], P[2]);
    }
  }
  if (in) {
    uint8_t* __restrict__ o = rgb_out + ((size_t)y * W + x) * 3;
    o[0] = (uint8_t)(c & 255u), o[1] = (uint8_t)((c >> 8) & 255u), o[2] = (uint8_t)((c >> 16) & 255u);
  }
  const int nc = __popcll(__ballot((c >> 24) != 0u)), nd = __popcll(__ballot(has));
  if (lane == 0) {
    if (nc > 0) atomicAdd(&info[1], nc);
    if (nd > 0) atomicAdd(&info[2], nd);
  }
}

// ---- the mesh -------------------------------------------------------------------------------------------------------------
#define MS_THREADS 256
#define MS_ROUNDS 2
#define MS_BLOCK (MS_THREADS * MS_ROUNDS)   // voxels a workgroup of ms_count_kernel and ms_emit_kernel walks
#define MS_BLOCK_SHIFT 9
#define MS_SCAN_THREADS 1024                // block totals a pass of ms_scan_kernel takes: one pass covers 2^19 voxels
#define MS_MAX_VOXELS (1 << 27)
#define MS_GRID 2048                        // workgroups of a pass over the voxels: 8 on each of the 256 CUs, each walks every 2048th block
// a voxel's record: its 7 live bits, then the vertices (12 bits) and the triangles (13 bits) of the voxels before it in its block
static_assert(MS_BLOCK == 1 << MS_BLOCK_SHIFT && (MS_BLOCK - 1) * 7 < (1 << 12) && (MS_BLOCK - 1) * 12 < (1 << 13), "the record is 7 + 12 + 13 bits");

// tetrahedron m of the Kuhn split: corners 0, k1, k2, 7 of the cell (corner b = x + 2 y + 4 z), the permutations of the axes in
// lexicographic order
__device__ __forceinline__ constexpr int ms_k1(int m) { return 1 << (m >> 1); }
__device__ __forceinline__ constexpr int ms_k2(int m) { return ms_k1(m) | 1 << (m == 0 ? 1 : m == 1 ? 2 : m == 2 ? 0 : m == 3 ? 2 : m == 4 ? 0 : 1); }
// bit 2 S + n: triangle n of sign pattern S leaves with its second and third vertex swapped.  One word for the even
// permutations and one for the odd: a reflection of the tetrahedron turns every triangle over.
__device__ __forceinline__ constexpr unsigned ms_swap(int m) { return (m == 0 || m == 3 || m == 4) ? 0x10710c10u : 0x070c71c4u; }

__device__ __forceinline__ unsigned ms_pattern(unsigned C, int m) {
  return (C & 1u) | ((C >> ms_k1(m)) & 1u) << 1 | ((C >> ms_k2(m)) & 1u) << 2 | ((C >> 7) & 1u) << 3;
}

// observed (bit 0) and inside (bit 1) of the voxels (j, k), (j + 1, k), (j, k + 1), (j + 1, k + 1) of column idx, two bits each;
// a voxel past the volume reads as unobserved
__device__ __forceinline__ unsigned ms_column(const float* __restrict__ tsdf, const float* __restrict__ weight, const TsGrid& g, int idx, int j, int k) {
  const int sy = g.Nx, sz = g.Nx * g.Ny;
  const bool hy = j < g.Ny - 1, hz = k < g.Nz - 1;
  unsigned c = (weight[idx] > 0.0f ? 1u : 0u) | (tsdf[idx] <= 0.0f ? 2u : 0u);
  if (hy) c |= ((weight[idx + sy] > 0.0f ? 1u : 0u) | (tsdf[idx + sy] <= 0.0f ? 2u : 0u)) << 2;
  if (hz) c |= ((weight[idx + sz] > 0.0f ? 1u : 0u) | (tsdf[idx + sz] <= 0.0f ? 2u : 0u)) << 4;
  if (hy && hz) c |= ((weight[idx + sz + sy] > 0.0f ? 1u : 0u) | (tsdf[idx + sz + sy] <= 0.0f ? 2u : 0u)) << 6;
  return c;
}

// code[v] of the cell whose low corner is voxel v: 0x100 | the inside bits of its 8 corners when it is valid, else 0
__global__ __launch_bounds__(MS_THREADS) void ms_classify_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight, TsGrid g,
                                                                 int nblk, uint16_t* __restrict__ code) {
  const int total = g.Nx * g.Ny * g.Nz, lane = threadIdx.x & 63;
  for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {   // uniform: every lane of a wavefront reaches the shuffle
    const int idx = blk * MS_THREADS + threadIdx.x;
    const bool in = idx < total;
    const int row = idx / g.Nx, i = idx - row * g.Nx, k = row / g.Ny, j = row - k * g.Ny;
    const bool has_x = in && i < g.Nx - 1;
    const unsigned mine = in ? ms_column(tsdf, weight, g, idx, j, k) : 0u;
    unsigned next = __shfl_down(mine, 1, 64);   // the next lane holds the column at x + 1; the last lane reads it
    if (lane == 63) next = has_x ? ms_column(tsdf, weight, g, idx + 1, j, k) : 0u;
    unsigned c = 0;
    if (has_x && j < g.Ny - 1 && k < g.Nz - 1 && (mine & next & 0x55u) == 0x55u) c = 0x100u | ((mine >> 1) & 0x55u) | (next & 0xAAu);
    if (in) code[idx] = (uint16_t)c;
  }
}

// edge (corner a, corner b) of a cell crosses and the cell is valid
__device__ __forceinline__ unsigned ms_cross(unsigned C, int a, int b) { return (C >> 8) & ((C >> a) ^ (C >> b)) & 1u; }

// the cell is valid with corners on both sides: only such a cell has a crossing edge
__device__ __forceinline__ unsigned ms_cut(unsigned C) { return (C >> 8) & ((((C & 0xffu) + 1u) & 0xfeu) != 0u ? 1u : 0u); }

__device__ __forceinline__ int ms_triangles(unsigned C) {
  if (!(C & 0x100u)) return 0;
  int n = 0;
#pragma unroll
  for (int m = 0; m < 6; ++m) {
    const int pc = __popc(ms_pattern(C, m));
    n += (pc == 0 || pc == 4) ? 0 : (pc == 2 ? 2 : 1);
  }
  return n;
}

__global__ __launch_bounds__(MS_THREADS) void ms_count_kernel(const uint16_t* __restrict__ code, TsGrid g, const int32_t* __restrict__ found,
                                                              int nblk, uint32_t* __restrict__ rec, int2* __restrict__ totals,
                                                              int32_t* __restrict__ info) {
  __shared__ int wave_sum[MS_ROUNDS * 4];
  __shared__ int wave_cells[4];
  const bool on = found ? found[0] != 0 : true;   // uniform
  const int total = g.Nx * g.Ny * g.Nz, sy = g.Nx, sz = g.Nx * g.Ny;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int cells = 0;               // the valid cells of this wavefront's voxels over the whole walk: the same in all of its lanes
  for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {   // uniform
    unsigned live[MS_ROUNDS];
    int packed[MS_ROUNDS], incl[MS_ROUNDS];   // vertices in the low half, triangles in the high half: at most 3584 and 6144 a block
#pragma unroll
    for (int r = 0; r < MS_ROUNDS; ++r) {
      const int idx = (blk * MS_ROUNDS + r) * MS_THREADS + threadIdx.x;
      unsigned lv = 0;
      int nt = 0;
      bool valid = false;
      if (idx < total && on) {
        const int row = idx / g.Nx, i = idx - row * g.Nx, k = row / g.Ny, j = row - k * g.Ny;
        const bool lx = i > 0, ly = j > 0, lz = k > 0;
        // the cells that hold an edge of this voxel: its own and those one step down along the axes the edge does not run along
        const unsigned C0 = code[idx], Cx = lx ? code[idx - 1] : 0u, Cy = ly ? code[idx - sy] : 0u, Cz = lz ? code[idx - sz] : 0u;
        const unsigned Cxy = lx && ly ? code[idx - 1 - sy] : 0u, Cxz = lx && lz ? code[idx - 1 - sz] : 0u, Cyz = ly && lz ? code[idx - sy - sz] : 0u;
        // most voxels lie away from the surface: no cell around them is cut, so none of their edges is live
        if (ms_cut(C0) | ms_cut(Cx) | ms_cut(Cy) | ms_cut(Cz) | ms_cut(Cxy) | ms_cut(Cxz) | ms_cut(Cyz)) {
          lv = (ms_cross(C0, 0, 1) | ms_cross(Cy, 2, 3) | ms_cross(Cz, 4, 5) | ms_cross(Cyz, 6, 7)) |
               (ms_cross(C0, 0, 2) | ms_cross(Cx, 1, 3) | ms_cross(Cz, 4, 6) | ms_cross(Cxz, 5, 7)) << 1 |
               (ms_cross(C0, 0, 3) | ms_cross(Cz, 4, 7)) << 2 |
               (ms_cross(C0, 0, 4) | ms_cross(Cx, 1, 5) | ms_cross(Cy, 2, 6) | ms_cross(Cxy, 3, 7)) << 3 |
               (ms_cross(C0, 0, 5) | ms_cross(Cy, 2, 7)) << 4 | (ms_cross(C0, 0, 6) | ms_cross(Cx, 1, 7)) << 5 | ms_cross(C0, 0, 7) << 6;
          nt = ms_triangles(C0);
        }
        valid = (C0 & 0x100u) != 0;
      }
      live[r] = lv;
      packed[r] = __popc(lv) | nt << 16;
      // a wavefront away from the surface has nothing to scan (uniform)
      incl[r] = __ballot(packed[r] != 0) != 0ull ? cotr_scan::wave_scan(packed[r]) : packed[r];
      cotr_scan::wave_sum_put(incl[r], wave_sum, r * 4 + wave);
      cells += __popcll(__ballot(valid));
    }
    __syncthreads();
    const int all = cotr_scan::wave_sums_below<MS_ROUNDS * 4>(wave_sum, MS_ROUNDS * 4);
    // a block with no vertex has no triangle either (a cut tetrahedron cuts an edge at q0, which its own voxel owns) and nobody
    // reads its records: ms_emit_kernel takes them as 0
    if (all != 0) {
#pragma unroll
      for (int r = 0; r < MS_ROUNDS; ++r) {
        const int idx = (blk * MS_ROUNDS + r) * MS_THREADS + threadIdx.x;
        const int ex = cotr_scan::wave_sums_below<MS_ROUNDS * 4>(wave_sum, r * 4 + wave) + incl[r] - packed[r];
        if (idx < total) rec[idx] = live[r] | (unsigned)(ex & 0xffff) << 7 | (unsigned)(ex >> 16) << 19;
      }
    }
    if (threadIdx.x == 0) totals[blk] = make_int2(all & 0xffff, all >> 16);
    __syncthreads();   // wave_sum is written again
  }
  if (lane == 0) wave_cells[wave] = cells;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int n = (wave_cells[0] + wave_cells[1]) + (wave_cells[2] + wave_cells[3]);
    if (n > 0) atomicAdd(&info[3], n);   // the call's only atomic
  }
}

// one workgroup: bases[b] = the vertices and triangles of the blocks before b, and both counts into info
__global__ __launch_bounds__(MS_SCAN_THREADS) void ms_scan_kernel(const int2* __restrict__ totals, int nblk, int2* __restrict__ bases,
                                                                  int32_t* __restrict__ info) {
  __shared__ int2 wave_sum[MS_SCAN_THREADS / 64];
  const int2 all = cotr_scan::scan_array<MS_SCAN_THREADS / 64>(
      nblk, wave_sum, [&](int b) { return totals[b]; }, [&](int b, int2 before) { bases[b] = before; });
  if (threadIdx.x == 0) info[1] = all.x, info[2] = all.y;
}

// the value at grid coordinates q by ts_trilinear's rule; false outside the box or at an unobserved corner
__device__ __forceinline__ bool ms_sample(const float* __restrict__ tsdf, const float* __restrict__ weight, const TsGrid& g, double qx, double qy,
                                          double qz, double* f) {
  const double q[3] = {qx, qy, qz};
  return ts_in_box(g, q) && ts_trilinear(tsdf, weight, g, q, f);
}

// the triangles of one tetrahedron with sign pattern S (1 .. 14) from the vertices on its six edges, rows `row` on
__device__ __forceinline__ int ms_tetrahedron(unsigned S, unsigned swap, int e01, int e02, int e03, int e12, int e13, int e23,
                                              int32_t* __restrict__ tris, int row, int cap) {
  int A, B, C, D = -1;       // (A, B, C), then with a second triangle (A, C, D)
  switch (S) {
    case 1: case 14: A = e01, B = e02, C = e03; break;
    case 2: case 13: A = e01, B = e12, C = e13; break;
    case 4: case 11: A = e02, B = e12, C = e23; break;
    case 8: case 7: A = e03, B = e13, C = e23; break;
    case 3: A = e02, B = e03, C = e13, D = e12; break;
    case 5: A = e01, B = e03, C = e23, D = e12; break;
    case 9: A = e01, B = e02, C = e23, D = e13; break;
    case 6: A = e01, B = e13, C = e23, D = e02; break;
    case 10: A = e01, B = e12, C = e23, D = e03; break;
    default: A = e02, B = e12, C = e13, D = e03; break;   // 12
  }
  const bool two = __popc(S) == 2;
  const unsigned sw = swap >> (2 * S);
  if (row < cap) {
    int32_t* t = tris + (size_t)row * 3;
    t[0] = A, t[1] = (sw & 1u) ? C : B, t[2] = (sw & 1u) ? B : C;
  }
  if (two && row + 1 < cap) {
    int32_t* t = tris + (size_t)(row + 1) * 3;
    t[0] = A, t[1] = (sw & 2u) ? D : C, t[2] = (sw & 2u) ? C : D;
  }
  return two ? 2 : 1;
}

// A workgroup whose block holds no vertex and no triangle leaves at once.  tsdf is read a second time here, at the two ends of
// the live edges only (and around them for the normals): a pass that kept the values of every voxel for this one would write
// 4 B a voxel to spare 8 B a vertex.
__global__ __launch_bounds__(MS_THREADS) void ms_emit_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight, TsGrid g,
                                                             const uint16_t* __restrict__ code, const uint32_t* __restrict__ rec,
                                                             int nblk, const int2* __restrict__ totals, const int2* __restrict__ bases,
                                                             double* __restrict__ verts, double* __restrict__ normals, int cap_verts,
                                                             int32_t* __restrict__ tris, int cap_tris) {
  const int total = g.Nx * g.Ny * g.Nz, sy = g.Nx, sz = g.Nx * g.Ny;
  for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    if (totals[blk].x == 0) continue;   // no vertex, so no triangle
    const int2 base = bases[blk];
#pragma unroll 1
    for (int r = 0; r < MS_ROUNDS; ++r) {
      const int idx = (blk * MS_ROUNDS + r) * MS_THREADS + threadIdx.x;
      if (idx >= total) continue;
      const unsigned me = rec[idx], live = me & 127u;
      const int row = idx / g.Nx, i = idx - row * g.Nx, k = row / g.Ny, j = row - k * g.Ny;
      if (live && cap_verts > 0) {
        const int first = base.x + (int)((me >> 7) & 4095u);
        const double fa = (double)tsdf[idx];
#pragma unroll
        for (int d = 1; d < 8; ++d) {
          const int slot = first + __popc(live & ((1u << (d - 1)) - 1u));
          if (!((live >> (d - 1)) & 1u) || slot >= cap_verts) continue;   // beyond the capacity: counted, not written
          const double fb = (double)tsdf[idx + (d & 1) + ((d >> 1) & 1) * sy + (d >> 2) * sz];
          const double t = fa / (fa - fb);
          const double gx = (d & 1) ? (double)i + t : (double)i, gy = (d & 2) ? (double)j + t : (double)j, gz = (d & 4) ? (double)k + t : (double)k;
          double* v = verts + (size_t)slot * 3;
          v[0] = g.ox + g.voxel * gx, v[1] = g.oy + g.voxel * gy, v[2] = g.oz + g.voxel * gz;
          if (normals) {
            double fp[3], fm[3];
            bool ok = ms_sample(tsdf, weight, g, gx + 1.0, gy, gz, &fp[0]) && ms_sample(tsdf, weight, g, gx - 1.0, gy, gz, &fm[0]);
            ok = ok && ms_sample(tsdf, weight, g, gx, gy + 1.0, gz, &fp[1]) && ms_sample(tsdf, weight, g, gx, gy - 1.0, gz, &fm[1]);
            ok = ok && ms_sample(tsdf, weight, g, gx, gy, gz + 1.0, &fp[2]) && ms_sample(tsdf, weight, g, gx, gy, gz - 1.0, &fm[2]);
            double n0 = NAN, n1 = NAN, n2 = NAN;
            if (ok) {
              const double Gx = fp[0] - fm[0], Gy = fp[1] - fm[1], Gz = fp[2] - fm[2];
              const double len = sqrt((Gx * Gx + Gy * Gy) + Gz * Gz);
              if (len > 0.0) n0 = Gx / len, n1 = Gy / len, n2 = Gz / len;   // false for NaN
            }
            double* n = normals + (size_t)slot * 3;
            n[0] = n0, n[1] = n1, n[2] = n2;
          }
        }
      }
      if (cap_tris <= 0) continue;
      const unsigned C = code[idx];
      if (!(C & 0x100u) || (C & 0xffu) == 0u || (C & 0xffu) == 0xffu) continue;
      // the first vertex and the live bits of the 7 corners that own an edge of this cell
      int cb[7];
      unsigned lv[7];
#pragma unroll
      for (int c = 0; c < 7; ++c) {
        const int u = idx + (c & 1) + ((c >> 1) & 1) * sy + (c >> 2) * sz;
        const int ub = u >> MS_BLOCK_SHIFT;
        const bool mine = ub == blk;
        const unsigned ru = c == 0 ? me : (mine || totals[ub].x != 0) ? rec[u] : 0u;   // a block without vertices wrote no records
        const int bu = mine ? base.x : bases[ub].x;
        cb[c] = bu + (int)((ru >> 7) & 4095u);
        lv[c] = ru & 127u;
      }
      int out = base.y + (int)(me >> 19);
#pragma unroll
      for (int m = 0; m < 6; ++m) {
        const unsigned S = ms_pattern(C, m);
        if (S == 0u || S == 15u) continue;
        constexpr int k0 = 0, k3 = 7;
        const int k1 = ms_k1(m), k2 = ms_k2(m);
        // the vertex on edge (corner a, corner b): the owner's first vertex + its live edges below dcode b - a
#define MS_EDGE(a, b) (cb[a] + __popc(lv[a] & ((1u << ((b) - (a) - 1)) - 1u)))
        out += ms_tetrahedron(S, ms_swap(m), MS_EDGE(k0, k1), MS_EDGE(k0, k2), MS_EDGE(k0, k3), MS_EDGE(k1, k2), MS_EDGE(k1, k3), MS_EDGE(k2, k3),
                              tris, out, cap_tris);
#undef MS_EDGE
      }
    }
  }
}

// the rows of tris past the count
__global__ __launch_bounds__(MS_THREADS) void ms_pad_kernel(int32_t* __restrict__ tris, int cap_tris, const int32_t* __restrict__ info) {
  const size_t e = (size_t)blockIdx.x * MS_THREADS + threadIdx.x;
  if (e < (size_t)cap_tris * 3 && e >= (size_t)info[2] * 3) tris[e] = -1;
}

// ---- host side ------------------------------------------------------------------------------------------------------------
namespace {

bool ts_finite(double v) { return fabs(v) < INFINITY; }   // false for NaN

const char* ts_check_dims(int Nx, int Ny, int Nz, double voxel) {
  if (Nx < 2 || Ny < 2 || Nz < 2 || (long long)Nx * Ny * Nz > TS_MAX_VOXELS) return "Nx, Ny and Nz must be >= 2 with at most 2^28 voxels";
  if (!(voxel > 0.0) || !ts_finite(voxel)) return "voxel must be finite and > 0";
  return nullptr;
}

// the volume's arguments -> g; the message of the first rule broken, or NULL
const char* ts_check_volume(const float* tsdf, const float* weight, int Nx, int Ny, int Nz, const double* origin, double voxel, TsGrid* g) {
  if (const char* msg = ts_check_dims(Nx, Ny, Nz, voxel)) return msg;
  if (!tsdf || !weight || !origin) return "tsdf, weight and origin must not be NULL";
  if (!ts_finite(origin[0]) || !ts_finite(origin[1]) || !ts_finite(origin[2])) return "origin must be finite";
  if (!aligned(tsdf, 4) || !aligned(weight, 4)) return "floats and int32 must be 4-byte and doubles 8-byte aligned";
  *g = {Nx, Ny, Nz, origin[0], origin[1], origin[2], voxel};
  return nullptr;
}

// the same for the colour volume, which is read and written 16 bytes at a time
const char* ts_check_color(const float* color, int Nx, int Ny, int Nz, const double* origin, double voxel, TsGrid* g) {
  if (const char* msg = ts_check_dims(Nx, Ny, Nz, voxel)) return msg;
  if (!color || !origin) return "color and origin must not be NULL";
  if (!ts_finite(origin[0]) || !ts_finite(origin[1]) || !ts_finite(origin[2])) return "origin must be finite";
  if (!aligned(color, 16)) return "color must be 16-byte aligned";
  *g = {Nx, Ny, Nz, origin[0], origin[1], origin[2], voxel};
  return nullptr;
}

// Ks and obs_weight of a call -> caps; the message of the first rule broken, or NULL
const char* ts_captures(const double* Ks, const double* obs_weight, int n, TsCaps* caps) {
  for (int c = 0; c < TS_MAX_CAPS; ++c) caps->w[c] = 1.0;
  es_cameras(Ks, 0, &caps->cams);   // every row at its default; a row's camera and weight are then checked together, in row order
  for (int c = 0; c < n; ++c) {
    if (!es_camera(Ks + c * 9, &caps->cams.k[c])) return ES_CAMERAS_WHAT;
    if (obs_weight) {
      if (!(obs_weight[c] > 0.0) || !ts_finite(obs_weight[c])) return "every obs_weight must be finite and > 0";
      caps->w[c] = obs_weight[c];
    }
  }
  return nullptr;
}

}  // namespace

extern "C" {

int cotr_tsdf_integrate(float* tsdf, float* weight, int Nx, int Ny, int Nz, const double* origin, double voxel, double trunc,
                        const float* depths, int n, int H, int W, const double* Ks, const double* c2w, const int32_t* found,
                        const double* obs_weight, double max_weight, int32_t* info_out, cotr_stream stream) {
  static const char* fn = "cotr_tsdf_integrate";
  TsGrid g;
  if (const char* msg = ts_check_volume(tsdf, weight, Nx, Ny, Nz, origin, voxel, &g)) return arg_fail(fn, msg);
  if (!(trunc > 0.0) || !ts_finite(trunc)) return arg_fail(fn, "trunc must be finite and > 0");
  if (n < 1 || n > TS_MAX_CAPS) return arg_fail(fn, "n must be in [1, 32]");
  if (H < 1 || W < 1 || (long long)H * W > MAX_PIXELS) return arg_fail(fn, "H and W must be >= 1 with at most 2^28 pixels");
  if (!(max_weight > 0.0)) return arg_fail(fn, "max_weight must be > 0");
  if (!depths || !Ks || !c2w || !info_out) return arg_fail(fn, "depths, Ks, c2w and info_out must not be NULL");
  TsCaps caps;
  if (const char* msg = ts_captures(Ks, obs_weight, n, &caps)) return arg_fail(fn, msg);
  if (!aligned(depths, 4) || !aligned(c2w, 8) || !aligned(found, 4) || !aligned(info_out, 4))
    return arg_fail(fn, "floats and int32 must be 4-byte and doubles 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int total = Nx * Ny * Nz, per_group = 256 * TS_ROWS;
  hipLaunchKernelGGL(hl_begin_kernel<>, dim3(1), dim3(64), 0, s, found, n, 4, info_out);
  hipLaunchKernelGGL(ts_integrate_kernel, dim3((unsigned)((total + per_group - 1) / per_group)), dim3(256), 0, s, tsdf, weight, g, trunc, depths, n, H,
                     W, caps, c2w, found, max_weight, info_out);
  return launched();
}

int cotr_tsdf_raycast(const float* tsdf, const float* weight, int Nx, int Ny, int Nz, const double* origin, double voxel, const double* K,
                      const double* c2w, const int32_t* found, int H, int W, double near, double far, double step, float* depth_out,
                      double* normal_out, int32_t* info_out, cotr_stream stream) {
  static const char* fn = "cotr_tsdf_raycast";
  TsGrid g;
  if (const char* msg = ts_check_volume(tsdf, weight, Nx, Ny, Nz, origin, voxel, &g)) return arg_fail(fn, msg);
  if (H < 1 || W < 1 || (long long)H * W > MAX_PIXELS) return arg_fail(fn, "H and W must be >= 1 with at most 2^28 pixels");
  if (!(near >= 0.0) || !ts_finite(near)) return arg_fail(fn, "near must be finite and >= 0");
  if (!(far > near) || !ts_finite(far)) return arg_fail(fn, "far must be finite and > near");
  if (!(step > 0.0) || !ts_finite(step)) return arg_fail(fn, "step must be finite and > 0");
  const double steps = ceil((far - near) / step);
  if (!(steps <= (double)TS_MAX_STEPS)) return arg_fail(fn, "ceil((far - near) / step) must be at most 65536");
  if (!K || !c2w || !depth_out || !info_out) return arg_fail(fn, "K, c2w, depth_out and info_out must not be NULL");
  TsRay ray;
  if (!es_camera(K, &ray.k)) return arg_fail(fn, "the camera matrix must be finite with focal lengths that are not 0");
  if (!aligned(c2w, 8) || !aligned(found, 4) || !aligned(depth_out, 4) || !aligned(normal_out, 8) || !aligned(info_out, 4))
    return arg_fail(fn, "floats and int32 must be 4-byte and doubles 8-byte aligned");
  ray.H = H, ray.W = W, ray.steps = (int)steps, ray.near = near, ray.step = step;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned tiles = (unsigned)((W + 15) / 16) * (unsigned)((H + 15) / 16);
  hipLaunchKernelGGL(hl_begin_kernel<>, dim3(1), dim3(64), 0, s, found, 1, 4, info_out);
  hipLaunchKernelGGL(ts_raycast_kernel, dim3(tiles), dim3(256), 0, s, tsdf, weight, g, ray, c2w, found, depth_out, normal_out, info_out);
  return launched();
}

int cotr_tsdf_color_integrate(float* color, int Nx, int Ny, int Nz, const double* origin, double voxel, double trunc, const float* depths,
                              const uint8_t* images, int n, int H, int W, const double* Ks, const double* c2w, const int32_t* found,
                              const double* obs_weight, double max_weight, int32_t* info_out, cotr_stream stream) {
  static const char* fn = "cotr_tsdf_color_integrate";
  TsGrid g;
  if (const char* msg = ts_check_color(color, Nx, Ny, Nz, origin, voxel, &g)) return arg_fail(fn, msg);
  if (!(trunc > 0.0) || !ts_finite(trunc)) return arg_fail(fn, "trunc must be finite and > 0");
  if (n < 1 || n > TS_MAX_CAPS) return arg_fail(fn, "n must be in [1, 32]");
  if (H < 1 || W < 1 || (long long)H * W > MAX_PIXELS) return arg_fail(fn, "H and W must be >= 1 with at most 2^28 pixels");
  if (!(max_weight > 0.0)) return arg_fail(fn, "max_weight must be > 0");
  if (!depths || !images || !Ks || !c2w || !info_out) return arg_fail(fn, "depths, images, Ks, c2w and info_out must not be NULL");
  TsCaps caps;
  if (const char* msg = ts_captures(Ks, obs_weight, n, &caps)) return arg_fail(fn, msg);
  if (!aligned(depths, 4) || !aligned(c2w, 8) || !aligned(found, 4) || !aligned(info_out, 4))
    return arg_fail(fn, "floats and int32 must be 4-byte and doubles 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int total = Nx * Ny * Nz, per_group = 256 * TS_ROWS;
  hipLaunchKernelGGL(hl_begin_kernel<>, dim3(1), dim3(64), 0, s, found, n, 4, info_out);
  hipLaunchKernelGGL(ts_color_integrate_kernel, dim3((unsigned)((total + per_group - 1) / per_group)), dim3(256), 0, s, reinterpret_cast<float4*>(color), g,
                     trunc, depths, images, n, H, W, caps, c2w, found, max_weight, info_out);
  return launched();
}

int cotr_tsdf_color_points(const float* color, int Nx, int Ny, int Nz, const double* origin, double voxel, const double* points, int n,
                           const int32_t* found, uint8_t* rgb_out, uint8_t* valid_out, int32_t* info_out, cotr_stream stream) {
  static const char* fn = "cotr_tsdf_color_points";
  TsGrid g;
  if (const char* msg = ts_check_color(color, Nx, Ny, Nz, origin, voxel, &g)) return arg_fail(fn, msg);
  if (n < 0 || n > TS_MAX_POINTS) return arg_fail(fn, "n must be in [0, 2^28]");
  if ((n > 0 && (!points || !rgb_out || !valid_out)) || !info_out)
    return arg_fail(fn, "points, rgb_out, valid_out (with n above 0) and info_out must not be NULL");
  if (!aligned(points, 8) || !aligned(found, 4) || !aligned(info_out, 4))
    return arg_fail(fn, "floats and int32 must be 4-byte and doubles 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(hl_begin_kernel<>, dim3(1), dim3(64), 0, s, found, 1, 4, info_out);
  if (n > 0)
    hipLaunchKernelGGL(ts_color_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const float4*>(color), g, points, n, found,
                       rgb_out, valid_out, info_out);
  return launched();
}

int cotr_tsdf_color_map(const float* color, int Nx, int Ny, int Nz, const double* origin, double voxel, const float* depth, int H, int W,
                        const double* K, const double* c2w, const int32_t* found, uint8_t* rgb_out, int32_t* info_out, cotr_stream stream) {
  static const char* fn = "cotr_tsdf_color_map";
  TsGrid g;
  if (const char* msg = ts_check_color(color, Nx, Ny, Nz, origin, voxel, &g)) return arg_fail(fn, msg);
  if (H < 1 || W < 1 || (long long)H * W > MAX_PIXELS) return arg_fail(fn, "H and W must be >= 1 with at most 2^28 pixels");
  if (!depth || !K || !c2w || !rgb_out || !info_out) return arg_fail(fn, "depth, K, c2w, rgb_out and info_out must not be NULL");
  EsCam cam;
  if (!es_camera(K, &cam)) return arg_fail(fn, "the camera matrix must be finite with focal lengths that are not 0");
  if (!aligned(depth, 4) || !aligned(c2w, 8) || !aligned(found, 4) || !aligned(info_out, 4))
    return arg_fail(fn, "floats and int32 must be 4-byte and doubles 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned tiles = (unsigned)((W + 15) / 16) * (unsigned)((H + 15) / 16);
  hipLaunchKernelGGL(hl_begin_kernel<>, dim3(1), dim3(64), 0, s, found, 1, 4, info_out);
  hipLaunchKernelGGL(ts_color_map_kernel, dim3(tiles), dim3(256), 0, s, reinterpret_cast<const float4*>(color), g, depth, cam, H, W, c2w, found, rgb_out,
                     info_out);
  return launched();
}

}  // extern "C"

namespace {

struct MsScratch {
  uint16_t* code;          // [voxels]
  uint32_t* rec;           // [voxels]
  int2 *totals, *bases;    // [nblk]
  size_t bytes;
  int nblk;
};

MsScratch ms_layout(void* base, int Nx, int Ny, int Nz) {
  const size_t total = (size_t)Nx * Ny * Nz;
  MsScratch L;
  Carver c(base);
  L.nblk = (int)((total + MS_BLOCK - 1) / MS_BLOCK);
  L.code = c.take<uint16_t>(total);
  L.rec = c.take<uint32_t>(total);
  L.totals = c.take<int2>(L.nblk);
  L.bases = c.take<int2>(L.nblk);
  L.bytes = c.bytes;
  return L;
}

const char* MS_DIMS = "Nx, Ny and Nz must be >= 2 with at most 2^27 voxels";

// each dimension first: the product of three ints can wrap a 64-bit integer
bool ms_dims_ok(int Nx, int Ny, int Nz) {
  return Nx >= 2 && Ny >= 2 && Nz >= 2 && Nx <= MS_MAX_VOXELS && Ny <= MS_MAX_VOXELS && Nz <= MS_MAX_VOXELS &&
         (long long)Nx * Ny <= MS_MAX_VOXELS && (long long)Nx * Ny * Nz <= MS_MAX_VOXELS;
}

}  // namespace

extern "C" {

int cotr_tsdf_mesh_scratch_bytes(int Nx, int Ny, int Nz, size_t* bytes) {
  static const char* fn = "cotr_tsdf_mesh_scratch_bytes";
  if (!bytes) return arg_fail(fn, "bytes must not be NULL");
  if (!ms_dims_ok(Nx, Ny, Nz)) return arg_fail(fn, MS_DIMS);
  *bytes = ms_layout(nullptr, Nx, Ny, Nz).bytes;
  return COTR_OK;
}

int cotr_tsdf_mesh(const float* tsdf, const float* weight, int Nx, int Ny, int Nz, const double* origin, double voxel, const int32_t* found,
                   double* verts_out, int cap_verts, double* normals_out, int32_t* tris_out, int cap_tris, int32_t* info_out, void* scratch,
                   size_t scratch_bytes, cotr_stream stream) {
  static const char* fn = "cotr_tsdf_mesh";
  TsGrid g;
  if (!ms_dims_ok(Nx, Ny, Nz)) return arg_fail(fn, MS_DIMS);
  if (const char* msg = ts_check_volume(tsdf, weight, Nx, Ny, Nz, origin, voxel, &g)) return arg_fail(fn, msg);
  if (cap_verts < 0 || cap_tris < 0) return arg_fail(fn, "cap_verts and cap_tris must be >= 0");
  if ((cap_verts > 0 && !verts_out) || (cap_tris > 0 && !tris_out) || !info_out)
    return arg_fail(fn, "verts_out, tris_out (with a capacity above 0) and info_out must not be NULL");
  if (!aligned(found, 4) || !aligned(verts_out, 8) || !aligned(normals_out, 8) || !aligned(tris_out, 4) || !aligned(info_out, 4))
    return arg_fail(fn, "floats and int32 must be 4-byte and doubles 8-byte aligned");
  const MsScratch L = ms_layout(scratch, Nx, Ny, Nz);
  if (!scratch || scratch_bytes < L.bytes || !aligned(scratch, 16))
    return arg_fail(fn, "scratch must be 16-byte aligned and hold cotr_tsdf_mesh_scratch_bytes(Nx, Ny, Nz) bytes");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int total = Nx * Ny * Nz;
  hipLaunchKernelGGL(hl_begin_kernel<>, dim3(1), dim3(64), 0, s, found, 1, 4, info_out);
  const int nrun = (total + MS_THREADS - 1) / MS_THREADS;
  hipLaunchKernelGGL(ms_classify_kernel, dim3((unsigned)std::min(nrun, MS_GRID)), dim3(MS_THREADS), 0, s, tsdf, weight, g, nrun, L.code);
  hipLaunchKernelGGL(ms_count_kernel, dim3((unsigned)std::min(L.nblk, MS_GRID)), dim3(MS_THREADS), 0, s, L.code, g, found, L.nblk, L.rec, L.totals, info_out);
  hipLaunchKernelGGL(ms_scan_kernel, dim3(1), dim3(MS_SCAN_THREADS), 0, s, L.totals, L.nblk, L.bases, info_out);
  if (cap_verts > 0 || cap_tris > 0)   // the blocks with a surface are few and heavy: a workgroup each, so that they spread over the CUs
    hipLaunchKernelGGL(ms_emit_kernel, dim3((unsigned)L.nblk), dim3(MS_THREADS), 0, s, tsdf, weight, g, L.code, L.rec, L.nblk, L.totals, L.bases, verts_out,
                       cap_verts > 0 ? normals_out : nullptr, cap_verts, tris_out, cap_tris);
  if (cap_tris > 0)
    hipLaunchKernelGGL(ms_pad_kernel, dim3((unsigned)(((size_t)cap_tris * 3 + MS_THREADS - 1) / MS_THREADS)), dim3(MS_THREADS), 0, s, tris_out, cap_tris,
                       info_out);
  return launched();
}

}  // extern "C"
