// Rasterisation of a triangle mesh with per-vertex 2-vectors into a dense [H,W,2] map: the device side of
// triangulate_corr (COTR/inference/inference_helper.py:293-308).  The reference draws the Delaunay triangles of
// the correspondences with OpenGL (vispy), B's normalised coordinates as vertex colours, into a float framebuffer
// of A's size; here the same picture is drawn by five launches on the caller's stream, with a coverage rule of our
// own that is exact and fully specified:
//   - vertices snapped to 1/256 px:  X = rint(u * W * 256), Y = rint(v * H * 256) (double, from the float32 input);
//     the sample of pixel (i, j) is (256 j + 128, 256 i + 128), the pixel centre;
//   - int64 edge functions of a triangle oriented so that 2A > 0; a sample is inside when every edge function is
//     > 0, or == 0 on an edge a->b with dy < 0 || (dy == 0 && dx > 0) (the sample moved by (eps, eps^2)): every
//     sample inside a proper triangulation is covered exactly once;
//   - where triangles overlap, the highest index wins (GL's draw order without a depth test): an atomicMax of
//     (index + 1) per sample, so the result does not depend on scheduling;
//   - value = sum of the three float32 attributes weighted by (edge function / 2A), evaluated in double and
//     rounded to float once; uncovered samples are 0.
// A triangle with an index outside [0, n_verts), a non-finite vertex, a snapped coordinate of magnitude >= 2^30
// (2^22 px; this keeps every edge function below 2^63) or zero snapped area covers nothing.
//
//   0. tri_clear_kernel   ids = 0 (a kernel, not a memset node: the same in every graph the call is captured into)
//   1. tri_setup_kernel   one thread per triangle: checks, snapping, orientation, bounding box of the samples it can
//                         cover (clipped to the canvas), cut into 16x16-sample tiles; the tile counts summed inside the block
//   2. tri_scan_kernel    one workgroup: the block totals summed (both by scan.h), and the total tile count
//   3. tri_raster_kernel  a fixed grid of wavefronts splits the total tile count into equal contiguous ranges (one
//                         binary search per wavefront, then a walk), so a sliver spanning the canvas is shared by
//                         many wavefronts; one 16x16 tile per wavefront step, 4 samples per lane, atomicMax of ids
//   4. tri_resolve_kernel one thread per pixel: interpolate the winning triangle, coalesced stores of out / mask
// No host waits, no allocation: capturable.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "handleless.h"
#include "scan.h"

using namespace cotr_detail;

#define TILE 16
#define SETUP_THREADS 256
#define RASTER_BLOCKS 1024
#define MAX_CANVAS 16384
#define COORD_LIMIT 1073741824.0   // 2^30 in 1/256 px

struct TriRec {         // 64 bytes
  int x[3], y[3];       // snapped vertices, oriented so that a2 > 0
  int vid[3];           // their vertex (attribute) indices in that order
  int i0, i1, j0, j1;   // sample rows / columns of the clipped bounding box
  int ntx;              // tiles across; 0: the triangle covers nothing
  long long a2;         // twice the signed area, > 0
};
static_assert(sizeof(TriRec) == 64, "TriRec layout");

// E_ab(p) = (b - a) x (p - a), exact: |coordinates| < 2^30, so both products stay below 2^62
__device__ __forceinline__ long long edge_fn(int ax, int ay, int bx, int by, long long px, long long py) {
  return ((long long)bx - ax) * (py - ay) - ((long long)by - ay) * (px - ax);
}

__device__ __forceinline__ bool edge_in(long long e, int ax, int ay, int bx, int by) {
  const int dx = bx - ax, dy = by - ay;   // |dx|, |dy| < 2^31
  return e > 0 || (e == 0 && (dy < 0 || (dy == 0 && dx > 0)));
}

__device__ __forceinline__ bool covers(const TriRec& r, long long px, long long py) {
  return edge_in(edge_fn(r.x[0], r.y[0], r.x[1], r.y[1], px, py), r.x[0], r.y[0], r.x[1], r.y[1]) &&
         edge_in(edge_fn(r.x[1], r.y[1], r.x[2], r.y[2], px, py), r.x[1], r.y[1], r.x[2], r.y[2]) &&
         edge_in(edge_fn(r.x[2], r.y[2], r.x[0], r.y[0], px, py), r.x[2], r.y[2], r.x[0], r.y[0]);
}

__device__ __forceinline__ long long tile_count(const TriRec& r) {
  return r.ntx == 0 ? 0 : (long long)r.ntx * ((r.i1 - r.i0) / TILE + 1);
}

__global__ __launch_bounds__(SETUP_THREADS) void tri_setup_kernel(const float* __restrict__ verts, int n_verts,
                                                                  const int32_t* __restrict__ tris, int n_tris, int H, int W,
                                                                  TriRec* __restrict__ recs, long long* __restrict__ local,
                                                                  long long* __restrict__ bsum) {
  __shared__ long long sums[SETUP_THREADS / 64];
  const int t = blockIdx.x * SETUP_THREADS + threadIdx.x;
  long long cnt = 0;
  if (t < n_tris) {
    TriRec r = {};
    int vid[3];
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
      vid[k] = tris[(size_t)t * 3 + k];
      ok = ok && vid[k] >= 0 && vid[k] < n_verts;
    }
    long long X[3] = {0, 0, 0}, Y[3] = {0, 0, 0};
    for (int k = 0; k < 3 && ok; ++k) {
      const double x = rint((double)verts[(size_t)vid[k] * 2] * (double)W * 256.0);
      const double y = rint((double)verts[(size_t)vid[k] * 2 + 1] * (double)H * 256.0);
      ok = fabs(x) < COORD_LIMIT && fabs(y) < COORD_LIMIT;   // false for NaN and inf as well
      if (ok) {
        X[k] = (long long)x;
        Y[k] = (long long)y;
      }
    }
    long long a2 = ok ? (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0]) : 0;
    if (a2 < 0) {
      long long tx = X[1], ty = Y[1];
      X[1] = X[2], Y[1] = Y[2], X[2] = tx, Y[2] = ty;
      const int tv = vid[1];
      vid[1] = vid[2], vid[2] = tv;
      a2 = -a2;
    }
    if (a2 > 0) {
      const long long xmin = min(X[0], min(X[1], X[2])), xmax = max(X[0], max(X[1], X[2]));
      const long long ymin = min(Y[0], min(Y[1], Y[2])), ymax = max(Y[0], max(Y[1], Y[2]));
      // samples 256 j + 128 within [xmin, xmax]; >> is floor division for negative values as well
      const long long j0 = max(-((128 - xmin) >> 8), 0LL), j1 = min((xmax - 128) >> 8, (long long)W - 1);
      const long long i0 = max(-((128 - ymin) >> 8), 0LL), i1 = min((ymax - 128) >> 8, (long long)H - 1);
      if (j0 <= j1 && i0 <= i1) {
        for (int k = 0; k < 3; ++k) {
          r.x[k] = (int)X[k];
          r.y[k] = (int)Y[k];
          r.vid[k] = vid[k];
        }
        r.i0 = (int)i0, r.i1 = (int)i1, r.j0 = (int)j0, r.j1 = (int)j1;
        r.ntx = (int)((j1 - j0) / TILE + 1);
        r.a2 = a2;
        cnt = tile_count(r);
      }
    }
    recs[t] = r;
  }
  long long total;
  const long long before = cotr_scan::block_scan<SETUP_THREADS / 64>(cnt, sums, &total);
  if (t < n_tris) local[t] = before + cnt;   // inclusive: incl_at reads it
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// bsum[0..nb) block totals -> exclusive block offsets; bsum[nb] = total tile count
__global__ __launch_bounds__(256) void tri_scan_kernel(long long* __restrict__ bsum, int nb) {
  __shared__ long long sums[4];
  const long long total = cotr_scan::scan_array<4>(
      nb, sums, [&](int b) { return bsum[b]; }, [&](int b, long long before) { bsum[b] = before; });
  if (threadIdx.x == 0) bsum[nb] = total;
}

__device__ __forceinline__ long long incl_at(const long long* local, const long long* boff, int t) {
  return local[t] + boff[t / SETUP_THREADS];
}

__global__ __launch_bounds__(256) void tri_raster_kernel(const TriRec* __restrict__ recs, const long long* __restrict__ local,
                                                         const long long* __restrict__ boff, int nb, int n_tris, int W,
                                                         int* __restrict__ ids) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  const long long nw = (long long)gridDim.x * 4;
  const long long total = boff[nb];
  const long long chunk = (total + nw - 1) / nw;
  const long long g0 = wave * chunk, g1 = min(g0 + chunk, total);
  if (g0 >= g1) return;
  // first triangle whose inclusive tile count exceeds g0
  int lo = 0, hi = n_tris - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (incl_at(local, boff, mid) > g0) hi = mid;
    else lo = mid + 1;
  }
  int t = lo;
  long long end = incl_at(local, boff, t);
  TriRec r = recs[t];
  long long start = end - tile_count(r);
  const int col = lane & 15, row = lane >> 4;
  for (long long g = g0; g < g1; ++g) {
    while (g >= end) {   // g < total = incl(n_tris - 1): t stays in range
      ++t;
      end = incl_at(local, boff, t);
      r = recs[t];
      start = end - tile_count(r);
    }
    const long long k = g - start;
    const int j = r.j0 + (int)(k % r.ntx) * TILE + col;
    const int ib = r.i0 + (int)(k / r.ntx) * TILE;
    if (j > r.j1) continue;
    const long long px = 256LL * j + 128;
#pragma unroll
    for (int s = 0; s < TILE / 4; ++s) {
      const int i = ib + row + 4 * s;
      if (i <= r.i1 && covers(r, px, 256LL * i + 128)) atomicMax(&ids[(size_t)i * W + j], t + 1);
    }
  }
}

__global__ __launch_bounds__(256) void tri_clear_kernel(int4* __restrict__ ids, long long n4) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k < n4) ids[k] = make_int4(0, 0, 0, 0);
}

__global__ __launch_bounds__(256) void tri_resolve_kernel(const TriRec* __restrict__ recs, const int* __restrict__ ids,
                                                          const float* __restrict__ attrs, int n_tris, int H, int W,
                                                          float2* __restrict__ out, uint8_t* __restrict__ mask) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long long)H * W) return;
  const int id = ids[p];
  const bool hit = id > 0 && id <= n_tris;   // (ids only ever holds 0 or a triangle index + 1; the bound keeps recs in range)
  float2 v = make_float2(0.f, 0.f);
  if (hit) {
    const TriRec r = recs[id - 1];
    const long long px = 256LL * (p % W) + 128, py = 256LL * (p / W) + 128;
    const double a2 = (double)r.a2;
    const double w[3] = {(double)edge_fn(r.x[1], r.y[1], r.x[2], r.y[2], px, py) / a2,
                         (double)edge_fn(r.x[2], r.y[2], r.x[0], r.y[0], px, py) / a2,
                         (double)edge_fn(r.x[0], r.y[0], r.x[1], r.y[1], px, py) / a2};
    double x = 0.0, y = 0.0;
    for (int k = 0; k < 3; ++k) {
      x += w[k] * (double)attrs[(size_t)r.vid[k] * 2];
      y += w[k] * (double)attrs[(size_t)r.vid[k] * 2 + 1];
    }
    v = make_float2((float)x, (float)y);
  }
  out[p] = v;
  if (mask) mask[p] = hit ? 1 : 0;
}

// ---- host side ------------------------------------------------------------------------------------------------------
namespace {

struct Layout {
  int* ids;           // [H][W], padded to whole int4
  TriRec* recs;       // [n_tris]
  long long* local;   // [n_tris]
  long long* bsum;    // [nb + 1]
  size_t bytes;
  int nb;
};

Layout layout(void* base, int n_tris, int H, int W) {
  Layout l;
  Carver c(base);
  l.nb = (n_tris + SETUP_THREADS - 1) / SETUP_THREADS;
  l.ids = c.take<int>((size_t)H * W);
  l.recs = c.take<TriRec>(n_tris);
  l.local = c.take<long long>(n_tris);
  l.bsum = c.take<long long>((size_t)l.nb + 1);
  l.bytes = c.bytes;
  return l;
}

const char* check_shape(int n_tris, int H, int W) {
  if (n_tris < 0) return "n_tris < 0";
  if (H < 1 || H > MAX_CANVAS || W < 1 || W > MAX_CANVAS) return "H and W must be in [1, 16384]";
  return nullptr;
}

}  // namespace

extern "C" {

int cotr_raster_mesh_scratch_bytes(int n_tris, int H, int W, size_t* bytes) {
  if (!bytes) return handleless_fail(COTR_ERR_ARG, "cotr_raster_mesh_scratch_bytes: bytes is NULL");
  if (const char* e = check_shape(n_tris, H, W)) return handleless_fail(COTR_ERR_ARG, e);
  *bytes = layout(nullptr, n_tris, H, W).bytes;
  return COTR_OK;
}

int cotr_raster_mesh(const float* verts, int n_verts, const float* attrs, const int32_t* tris, int n_tris, int H, int W,
                     float* out, uint8_t* mask, void* scratch, size_t scratch_bytes, cotr_stream stream) {
  if (const char* e = check_shape(n_tris, H, W)) return handleless_fail(COTR_ERR_ARG, e);
  if (n_verts < 0) return handleless_fail(COTR_ERR_ARG, "n_verts < 0");
  if (!out || !scratch) return handleless_fail(COTR_ERR_ARG, "out and scratch must not be NULL");
  if (n_tris > 0 && (!verts || !attrs || !tris)) return handleless_fail(COTR_ERR_ARG, "verts, attrs and tris must not be NULL");
  if (!aligned(scratch, 16) || !aligned(out, 8))
    return handleless_fail(COTR_ERR_ARG, "scratch must be 16-byte and out 8-byte aligned");
  const Layout l = layout(scratch, n_tris, H, W);
  if (scratch_bytes < l.bytes) return handleless_fail(COTR_ERR_ARG, "scratch is smaller than cotr_raster_mesh_scratch_bytes");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long npx = (long long)H * W, n4 = (npx + 3) / 4;   // the ids region is padded to 256 bytes: n4 int4 fit
  hipLaunchKernelGGL(tri_clear_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, reinterpret_cast<int4*>(l.ids), n4);
  if (n_tris > 0) {
    hipLaunchKernelGGL(tri_setup_kernel, dim3(l.nb), dim3(SETUP_THREADS), 0, s, verts, n_verts, tris, n_tris, H, W, l.recs, l.local, l.bsum);
    hipLaunchKernelGGL(tri_scan_kernel, dim3(1), dim3(256), 0, s, l.bsum, l.nb);
    hipLaunchKernelGGL(tri_raster_kernel, dim3(RASTER_BLOCKS), dim3(256), 0, s, l.recs, l.local, l.bsum, l.nb, n_tris, W, l.ids);
  }
  hipLaunchKernelGGL(tri_resolve_kernel, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, s, l.recs, l.ids, attrs, n_tris, H, W,
                     reinterpret_cast<float2*>(out), mask);
  return launched();
}

}  // extern "C"
