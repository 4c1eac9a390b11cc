// Overlap of the captures of a scene: the device side of cotr_amd/scene.py, which replaces the numpy of
// scripts/prepare_nn_distance_mat.py (distance_between_two_caps) and Capture.point_cloud_world.  Rule in DESIGN.md 3k.
//
// overlap(q, d), everything in double unless said otherwise, products and sums in this order, not contracted:
//   world points of d (cotr_world_points, once per capture), per pixel (x, y) in row-major order, z = depth_d[y, x]:
//     pixel_to_world of camera.h; w.xyz is stored as FLOAT32 (the reference's DEFAULT_PRECISION), an invalid pixel stores NaN
//   splat: X = the float32 point widened, project_inside of camera.h with P_q and the size of q; a kept point lands on
//     ix = clip(rint(u)), iy = clip(rint(v))
//     (ties to even).  The canvas pixel belongs to the kept point with the LARGEST source index y Wd + x landing there
//     (numpy's fancy assignment keeps the last writer; there is no depth test): atomicMax of index + 1 on a zeroed
//     uint32 canvas, which is independent of the order of arrival, so two runs give the same bytes.
//   score: per canvas pixel, canvas = the winner's p.z recomputed from its world point (the same operations on the same
//     operands), rm = a point landed, qm = depth_q > 0; union = #(qm | rm), good = #(qm & rm & |depth_q - canvas| < 1).
//     The two counts are integers: wave ballots, one pair of integer atomic adds per workgroup.
//   finalise: ratio = float(good / union) in double, 0 when union == 0.
// Pairs are processed in tiles of as many canvases as the caller's scratch holds; the launches of a tile are
// memset, splat, score.  Memory- and atomic-bound; float64 VALU, no MFMA.  No host waits, no allocation: capturable.
// Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "camera.h"
#include "handleless.h"

using namespace cotr_detail;

#define OV_THREADS 256
#define OV_WAVES (OV_THREADS / 64)

namespace {

struct OvCap {
  const float* depth;
  const float* xyz;
  int h, w, npx;
};

// a capture's table rows; npx is 0 for a capture the launch was not sized for (more than max_px pixels) or without a map
__device__ __forceinline__ OvCap load_cap(const unsigned long long* __restrict__ caps, const int32_t* __restrict__ shapes, int c, int max_px) {
  OvCap o;
  o.depth = reinterpret_cast<const float*>(caps[2 * c]);
  o.xyz = reinterpret_cast<const float*>(caps[2 * c + 1]);
  o.h = shapes[2 * c], o.w = shapes[2 * c + 1];
  const long long px = (long long)max(o.h, 0) * max(o.w, 0);
  o.npx = (o.depth && px <= (long long)max_px) ? (int)px : 0;
  return o;
}

// cams = Kinv[9] | c2w[16] per capture
__global__ __launch_bounds__(OV_THREADS) void world_points_kernel(const unsigned long long* __restrict__ caps,
                                                                  const int32_t* __restrict__ shapes, const double* __restrict__ cams,
                                                                  int max_px) {
  const int c = blockIdx.y;
  const OvCap cap = load_cap(caps, shapes, c, max_px);
  const int i = blockIdx.x * OV_THREADS + threadIdx.x;
  if (i >= cap.npx || !cap.xyz) return;
  const double* k = cams + 25 * (size_t)c;
  const float nan = __builtin_nanf("");
  float o0 = nan, o1 = nan, o2 = nan;
  double w[3];
  if (pixel_to_world(k, k + 9, (double)(i % cap.w), (double)(i / cap.w), (double)cap.depth[i], w))
    o0 = (float)w[0], o1 = (float)w[1], o2 = (float)w[2];
  float* out = const_cast<float*>(cap.xyz) + 3 * (size_t)i;
  out[0] = o0, out[1] = o1, out[2] = o2;
}

struct OvPair {
  OvCap q, d;
  const double* P;   // of q
  bool ok;
};

__device__ __forceinline__ OvPair load_pair(const unsigned long long* __restrict__ caps, const int32_t* __restrict__ shapes,
                                            const double* __restrict__ proj, const int32_t* __restrict__ pairs, int pair, int n_caps,
                                            int max_px) {
  OvPair p;
  const int q = pairs[2 * pair], d = pairs[2 * pair + 1];
  p.ok = q >= 0 && q < n_caps && d >= 0 && d < n_caps;
  if (!p.ok) {
    p.q = p.d = OvCap{nullptr, nullptr, 0, 0, 0};
    p.P = proj;
    return p;
  }
  p.q = load_cap(caps, shapes, q, max_px);
  p.d = load_cap(caps, shapes, d, max_px);
  if (!p.d.xyz) p.d.npx = 0;
  p.P = proj + 12 * (size_t)q;
  return p;
}

// grid (blocks of source points, pairs of the tile); win = the tile's canvases, max_px uint32 each
__global__ __launch_bounds__(OV_THREADS) void overlap_splat_kernel(const unsigned long long* __restrict__ caps,
                                                                   const int32_t* __restrict__ shapes, const double* __restrict__ proj,
                                                                   const int32_t* __restrict__ pairs, int first, int n_caps, int max_px,
                                                                   unsigned int* __restrict__ win) {
  const OvPair p = load_pair(caps, shapes, proj, pairs, first + blockIdx.y, n_caps, max_px);
  const int i = blockIdx.x * OV_THREADS + threadIdx.x;
  if (i >= p.d.npx || p.q.npx == 0) return;
  const float* X = p.d.xyz + 3 * (size_t)i;
  const float fz = X[2];
  if (fz != fz) return;                                   // an invalid pixel of d
  const double Xd[3] = {(double)X[0], (double)X[1], (double)fz};
  double u, v, pz;
  if (!project_inside(p.P, Xd, p.q.w, p.q.h, u, v, pz)) return;
  const int ix = min(max((int)rint(u), 0), p.q.w - 1), iy = min(max((int)rint(v), 0), p.q.h - 1);
  atomicMax(win + (size_t)blockIdx.y * max_px + (size_t)iy * p.q.w + ix, (unsigned int)i + 1u);
}

// grid (blocks of canvas pixels, pairs of the tile); counts [n_pairs][2] = (good, union), zeroed before the first tile
__global__ __launch_bounds__(OV_THREADS) void overlap_score_kernel(const unsigned long long* __restrict__ caps,
                                                                   const int32_t* __restrict__ shapes, const double* __restrict__ proj,
                                                                   const int32_t* __restrict__ pairs, int first, int n_caps, int max_px,
                                                                   const unsigned int* __restrict__ win, int32_t* __restrict__ counts) {
  __shared__ int part[OV_WAVES][2];
  const int pair = first + blockIdx.y;
  const OvPair p = load_pair(caps, shapes, proj, pairs, pair, n_caps, max_px);
  if ((int)blockIdx.x * OV_THREADS >= p.q.npx) return;    // the whole block
  const int i = blockIdx.x * OV_THREADS + threadIdx.x;
  bool good = false, uni = false;
  if (i < p.q.npx) {
    unsigned int w = win[(size_t)blockIdx.y * max_px + i];
    if (w > (unsigned int)p.d.npx) w = 0;                 // cannot happen on a canvas the splat wrote
    const float dq = p.q.depth[i];
    const bool qm = dq > 0.f, rm = w != 0;
    uni = qm || rm;
    if (qm && rm) {
      const float* X = p.d.xyz + 3 * (size_t)(w - 1);
      const double canvas = row4(p.P + 8, (double)X[0], (double)X[1], (double)X[2]);
      good = fabs((double)dq - canvas) < 1.0;
    }
  }
  const int g = __popcll(__ballot(good)), n = __popcll(__ballot(uni));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][0] = g, part[threadIdx.x >> 6][1] = n;
  __syncthreads();
  if (threadIdx.x < 2) {
    int s = 0;
#pragma unroll
    for (int k = 0; k < OV_WAVES; ++k) s += part[k][threadIdx.x];
    if (s) atomicAdd(counts + 2 * (size_t)pair + threadIdx.x, s);
  }
}

__global__ __launch_bounds__(OV_THREADS) void overlap_ratio_kernel(const int32_t* __restrict__ counts, int n_pairs, float* __restrict__ ratio) {
  const int i = blockIdx.x * OV_THREADS + threadIdx.x;
  if (i >= n_pairs) return;
  const int good = counts[2 * i], uni = counts[2 * i + 1];
  ratio[i] = uni > 0 ? (float)((double)good / (double)uni) : 0.f;
}

int blocks_for(int max_px) { return (max_px + OV_THREADS - 1) / OV_THREADS; }

size_t canvas_bytes(int max_px) { return ((size_t)max_px * sizeof(unsigned int) + 15) / 16 * 16; }

}  // namespace

extern "C" {

int cotr_world_points(const uint64_t* caps, const int32_t* shapes, const double* cams, int n, int max_px, cotr_stream stream) {
  if (n < 0 || n > MAX_ITEMS) return handleless_fail(COTR_ERR_ARG, "n must be in [0, 65535]");
  if (n == 0) return COTR_OK;
  if (max_px < 1 || max_px > MAX_PIXELS) return handleless_fail(COTR_ERR_ARG, "max_px must be in [1, 2^28]");
  if (!caps || !shapes || !cams) return handleless_fail(COTR_ERR_ARG, "the capture tables must not be NULL");
  if (!aligned(caps, 8) || !aligned(cams, 8)) return handleless_fail(COTR_ERR_ARG, "caps and cams must be 8-byte aligned");
  hipLaunchKernelGGL(world_points_kernel, dim3(blocks_for(max_px), n), dim3(OV_THREADS), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const unsigned long long*>(caps), shapes, cams, max_px);
  return launched();
}

size_t cotr_overlap_scratch(int pairs_in_flight, int max_px) {
  return pairs_in_flight > 0 && pairs_in_flight <= MAX_ITEMS && max_px > 0 && max_px <= MAX_PIXELS
             ? (size_t)pairs_in_flight * canvas_bytes(max_px) : 0;
}

int cotr_overlap_pairs(const uint64_t* caps, const int32_t* shapes, const double* proj, int n_caps, const int32_t* pairs, int n_pairs,
                       int max_px, float* ratio, int32_t* counts, void* scratch, size_t scratch_bytes, cotr_stream stream) {
  if (n_pairs < 0 || n_pairs > (1 << 24)) return handleless_fail(COTR_ERR_ARG, "n_pairs must be in [0, 2^24]");
  if (n_pairs == 0) return COTR_OK;
  if (n_caps < 1 || n_caps > MAX_ITEMS) return handleless_fail(COTR_ERR_ARG, "n_caps must be in [1, 65535]");
  if (max_px < 1 || max_px > MAX_PIXELS) return handleless_fail(COTR_ERR_ARG, "max_px must be in [1, 2^28]");
  if (!caps || !shapes || !proj || !pairs || !ratio || !counts)
    return handleless_fail(COTR_ERR_ARG, "the capture tables, pairs, ratio and counts must not be NULL");
  if (!aligned(caps, 8) || !aligned(proj, 8) || !aligned(scratch, 16))
    return handleless_fail(COTR_ERR_ARG, "caps and proj must be 8-byte, scratch 16-byte aligned");
  const size_t per = canvas_bytes(max_px);
  if (!scratch || scratch_bytes < per) return handleless_fail(COTR_ERR_ARG, "scratch is NULL or smaller than cotr_overlap_scratch(1, max_px)");
  const int tile = (int)(scratch_bytes / per < (size_t)MAX_ITEMS ? scratch_bytes / per : (size_t)MAX_ITEMS);
  const int nb = blocks_for(max_px);
  const unsigned long long* c = reinterpret_cast<const unsigned long long*>(caps);
  unsigned int* win = static_cast<unsigned int*>(scratch);
  const size_t stride = per / sizeof(unsigned int);       // canvases start 16-byte aligned
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_pairs * 2 * sizeof(int32_t), s);
  for (int first = 0; first < n_pairs && e == hipSuccess; first += tile) {
    const int t = n_pairs - first < tile ? n_pairs - first : tile;
    e = hipMemsetAsync(win, 0, (size_t)t * per, s);
    if (e != hipSuccess) break;
    hipLaunchKernelGGL(overlap_splat_kernel, dim3(nb, t), dim3(OV_THREADS), 0, s, c, shapes, proj, pairs, first, n_caps, (int)stride, win);
    hipLaunchKernelGGL(overlap_score_kernel, dim3(nb, t), dim3(OV_THREADS), 0, s, c, shapes, proj, pairs, first, n_caps, (int)stride, win, counts);
  }
  if (e != hipSuccess) return handleless_fail(COTR_ERR_HIP, hipGetErrorString(e));
  hipLaunchKernelGGL(overlap_ratio_kernel, dim3((n_pairs + OV_THREADS - 1) / OV_THREADS), dim3(OV_THREADS), 0, s, counts, n_pairs, ratio);
  return launched();
}

}  // extern "C"
