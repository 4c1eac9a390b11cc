// Ground-truth correspondences from depth and camera poses: the device side of cotr_amd/data.py, which replaces the numpy
// of COTR/datasets/cotr_dataset.py (get_corrs, the seed search, the zoomed captures) and COTR/projector/pcd_projector.py.
// Rules in DESIGN.md 3j.
//
// cotr_depth_corrs, per source pixel (x, y) with z = from_depth[y, x]: the camera rule of camera.h (pixel -> world point -> pixel
// (u, v) of the target and its depth p.z), then
//   zt = to_depth[floor(v), floor(u)]                                    keep iff |zt - p.z| < 0.5
// The kept rows (x, y, u, v) leave in SOURCE order (row-major pixels, or the order of the subset list): what the reference's
// chained boolean masks return.  A kept row's slot comes from scan.h, so two runs give the same bytes:
//   flags   one lane per source pixel: the predicate, a 64-bit wave ballot per wavefront to scratch
//   scan    one workgroup per item: the kept rows of each block (its four ballots) summed over the blocks before it, the count
//   scatter a kept lane's slot = its block's offset + the popcounts of the ballots before it + that of the lanes below it
// cotr_depth_valid is the same machinery with the predicate depth > 0 and the pixel index as the row.
// cotr_crop_depth_nearest is Pillow's NEAREST resize (ImagingScaleAffine): source column of output column j is
// int(xo_j), xo_0 = a / 2, xo_{j+1} = xo_j + a, a = size / out in double - the ACCUMULATED sum, not (j + 0.5) a.
// Memory-bound and small; float64 VALU, no MFMA.  No host waits, no allocation: capturable.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "camera.h"
#include "handleless.h"
#include "scan.h"

using namespace cotr_detail;

#define RP_THREADS 256
#define RP_WAVES (RP_THREADS / 64)
#define CROP_MAX_OUT 4096
#define CROP_ROWS 8
static_assert(RP_THREADS % 64 == 0 && RP_WAVES == 4, "four ballots per block (scan and scatter read them as a group)");

struct RpItem {
  const float* from;
  const float* to;
  const int32_t* subset;
  int hf, wf, ht, wt, n_src;
};

// the item's table rows; n_src never exceeds what the grid and the scratch were sized for, nor the source map
__device__ __forceinline__ RpItem load_item(const unsigned long long* __restrict__ ptrs, const int32_t* __restrict__ shapes, int item,
                                            int max_src) {
  RpItem it;
  it.from = reinterpret_cast<const float*>(ptrs[3 * item]);
  it.to = reinterpret_cast<const float*>(ptrs[3 * item + 1]);
  it.subset = reinterpret_cast<const int32_t*>(ptrs[3 * item + 2]);
  const int32_t* s = shapes + 5 * item;
  it.hf = s[0], it.wf = s[1], it.ht = s[2], it.wt = s[3];
  int n = min(max(s[4], 0), max_src);
  const long long px = (long long)max(it.hf, 0) * max(it.wf, 0);
  if (!it.subset && n > px) n = (int)px;
  if (!it.from || px == 0) n = 0;
  it.n_src = n;
  return it;
}

// source pixel index of lane i (< n_src), -1 when a subset entry points outside the map
__device__ __forceinline__ int source_index(const RpItem& it, int i) {
  if (!it.subset) return i;
  const int idx = it.subset[i];
  return (idx >= 0 && (long long)idx < (long long)it.hf * it.wf) ? idx : -1;
}

// the rule of the header; cam = Kinv[9] | c2w[16] | P_to[12]
__device__ __forceinline__ bool reproject(const RpItem& it, const double* __restrict__ cam, int idx, double& u, double& v) {
  u = v = 0.0;
  if (idx < 0 || !it.to || it.ht < 1 || it.wt < 1) return false;
  double w[3], pz;
  if (!pixel_to_world(cam, cam + 9, (double)(idx % it.wf), (double)(idx / it.wf), (double)it.from[idx], w)) return false;
  if (!project_inside(cam + 25, w, it.wt, it.ht, u, v, pz)) return false;
  const double zt = (double)it.to[(size_t)(int)floor(v) * it.wt + (int)floor(u)];                      // inside: 0 <= floor < size - 1
  return fabs(zt - pz) < 0.5;
}

// VALID: the predicate is depth > 0 and no camera is read
template <bool VALID>
__device__ __forceinline__ bool keep_lane(const RpItem& it, const double* __restrict__ cam, int idx, double& u, double& v) {
  if (VALID) {
    u = v = 0.0;
    return idx >= 0 && it.from[idx] > 0.f;
  }
  return reproject(it, cam, idx, u, v);
}

template <bool VALID>
__global__ __launch_bounds__(RP_THREADS) void reproj_flags_kernel(const unsigned long long* __restrict__ ptrs,
                                                                  const int32_t* __restrict__ shapes, const double* __restrict__ cams,
                                                                  int max_src, int nb_max, unsigned long long* __restrict__ ballots) {
  const int item = blockIdx.y;
  const RpItem it = load_item(ptrs, shapes, item, max_src);
  const int i = blockIdx.x * RP_THREADS + threadIdx.x;
  if ((int)blockIdx.x * RP_THREADS >= it.n_src) return;   // the whole block: scan and scatter stop at the same block
  double u, v;
  const bool keep = i < it.n_src && keep_lane<VALID>(it, VALID ? nullptr : cams + 37 * (size_t)item, source_index(it, i), u, v);
  const unsigned long long b = __ballot(keep);
  if ((threadIdx.x & 63) == 0) ballots[((size_t)item * nb_max + blockIdx.x) * RP_WAVES + (threadIdx.x >> 6)] = b;
}

__device__ __forceinline__ int block_kept(const unsigned long long* __restrict__ b) {
  return __popcll(b[0]) + __popcll(b[1]) + __popcll(b[2]) + __popcll(b[3]);
}

// one workgroup per item: offsets[block] = kept rows in the blocks before it, counts[item] = all of them
__global__ __launch_bounds__(RP_THREADS) void reproj_scan_kernel(const unsigned long long* __restrict__ ptrs,
                                                                 const int32_t* __restrict__ shapes, int max_src, int nb_max,
                                                                 const unsigned long long* __restrict__ ballots,
                                                                 int32_t* __restrict__ offsets, int32_t* __restrict__ counts) {
  __shared__ int wave_sum[RP_WAVES];
  const int item = blockIdx.x;
  const RpItem it = load_item(ptrs, shapes, item, max_src);
  const int nb = (it.n_src + RP_THREADS - 1) / RP_THREADS;
  const size_t first = (size_t)item * nb_max;
  const int total = cotr_scan::scan_array<RP_WAVES>(
      nb, wave_sum, [&](int b) { return block_kept(ballots + (first + b) * RP_WAVES); },
      [&](int b, int before) { offsets[first + b] = before; });
  if (threadIdx.x == 0) counts[item] = total;
}

template <bool VALID>
__global__ __launch_bounds__(RP_THREADS) void reproj_scatter_kernel(const unsigned long long* __restrict__ ptrs,
                                                                    const int32_t* __restrict__ shapes, const double* __restrict__ cams,
                                                                    int max_src, int nb_max,
                                                                    const unsigned long long* __restrict__ ballots,
                                                                    const int32_t* __restrict__ offsets, void* __restrict__ out, int cap) {
  const int item = blockIdx.y;
  const RpItem it = load_item(ptrs, shapes, item, max_src);
  if ((int)blockIdx.x * RP_THREADS >= it.n_src) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long* b = ballots + ((size_t)item * nb_max + blockIdx.x) * RP_WAVES;
  const unsigned long long mine = b[wave];
  if (!((mine >> lane) & 1)) return;
  int slot = offsets[(size_t)item * nb_max + blockIdx.x] + __popcll(mine & ((1ull << lane) - 1));
#pragma unroll
  for (int k = 0; k < RP_WAVES; ++k) slot += k < wave ? __popcll(b[k]) : 0;
  if (slot >= cap) return;                       // counted, not written
  const int idx = source_index(it, blockIdx.x * RP_THREADS + threadIdx.x);   // a kept lane: inside n_src and the map
  if (VALID) {
    static_cast<int32_t*>(out)[(size_t)item * cap + slot] = idx;
  } else {
    double u, v;
    reproject(it, cams + 37 * (size_t)item, idx, u, v);   // the same operations on the same operands as in the flags pass
    double2* row = static_cast<double2*>(out) + ((size_t)item * cap + slot) * 2;
    row[0] = make_double2((double)(idx % it.wf), (double)(idx / it.wf));
    row[1] = make_double2(u, v);
  }
}

// Pillow's ImagingScaleAffine for a crop: CROP_ROWS output rows x `out` columns of one item per workgroup.
// The index tables are Pillow's accumulated sums, so each is a serial chain of float64 additions: every workgroup rebuilds the
// column table (`out` additions on one lane) while another lane walks the row sum up to its own rows - out / CROP_ROWS
// workgroups per item repeat that prologue.  At out = 256 it is 256 dependent additions (about a microsecond) in front of a
// copy that is itself a few microseconds for a batch, and it keeps the entry point at one launch with no scratch; a table
// kernel in front would only pay from `out` in the thousands.  LDS: (out + CROP_ROWS) ints, sized by the launch.
__global__ __launch_bounds__(RP_THREADS) void crop_depth_nearest_kernel(const unsigned long long* __restrict__ srcs,
                                                                        const int32_t* __restrict__ shapes,
                                                                        const int32_t* __restrict__ boxes, float* __restrict__ dst, int out) {
  extern __shared__ int crop_tab[];
  int* xtab = crop_tab;
  int* ytab = crop_tab + out;
  const int item = blockIdx.y;
  const float* src = reinterpret_cast<const float*>(srcs[item]);
  const int H = shapes[2 * item], W = shapes[2 * item + 1];
  const int bx = boxes[3 * item], by = boxes[3 * item + 1], size = max(boxes[3 * item + 2], 1);
  const int y0 = blockIdx.x * CROP_ROWS;
  const double a = (double)size / (double)out;
  // the sums are sequential by Pillow's definition: one lane each for the columns and for the rows (out <= 4096 additions)
  if (threadIdx.x == 0) {
    double xo = a * 0.5;
    for (int j = 0; j < out; ++j) {
      xtab[j] = min((int)xo, size - 1);
      xo += a;
    }
  } else if (threadIdx.x == 64) {
    double yo = a * 0.5;
    for (int i = 0; i < y0 + CROP_ROWS && i < out; ++i) {
      if (i >= y0) ytab[i - y0] = min((int)yo, size - 1);
      yo += a;
    }
  }
  __syncthreads();
  if (!src || H < 1 || W < 1) return;
  for (int r = 0; r < CROP_ROWS && y0 + r < out; ++r) {
    const int yi = min(max(by + ytab[r], 0), H - 1);     // a box inside the map is never clamped
    const float* row = src + (size_t)yi * W;
    float* o = dst + ((size_t)item * out + y0 + r) * out;
    for (int j = threadIdx.x; j < out; j += RP_THREADS) o[j] = row[min(max(bx + xtab[j], 0), W - 1)];
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------
namespace {

int nb_for(int max_src) { return (max_src + RP_THREADS - 1) / RP_THREADS; }

size_t scratch_for(int n, int max_src) {
  const size_t blocks = (size_t)n * nb_for(max_src);
  return (blocks * (RP_WAVES * sizeof(unsigned long long) + sizeof(int32_t)) + 15) / 16 * 16;
}

template <bool VALID>
int compact(const uint64_t* ptrs, const int32_t* shapes, const double* cams, int n, int max_src, void* out, int cap, int32_t* counts,
            void* scratch, size_t scratch_bytes, cotr_stream stream) {
  if (n < 0 || n > MAX_ITEMS) return handleless_fail(COTR_ERR_ARG, "n must be in [0, 65535]");
  if (n == 0) return COTR_OK;
  if (max_src < 1 || max_src > MAX_PIXELS) return handleless_fail(COTR_ERR_ARG, "max_src must be in [1, 2^28]");
  if (cap < 0 || (size_t)n * cap > ((size_t)1 << 31)) return handleless_fail(COTR_ERR_ARG, "cap must be >= 0 and n * cap <= 2^31");
  if (!ptrs || !shapes || (!VALID && !cams) || !counts || (cap > 0 && !out))
    return handleless_fail(COTR_ERR_ARG, "the item tables, counts and the output must not be NULL");
  // rows are written as double2 pairs, indices one int32 at a time: each is asked for what its store needs
  if (!aligned(ptrs, 8) || !aligned(cams, 8) || !aligned(shapes, 4) || !aligned(counts, 4) || !aligned(out, VALID ? 4 : 16) || !aligned(scratch, 16))
    return handleless_fail(COTR_ERR_ARG, VALID ? "cotr_depth_valid: ptrs must be 8-byte, shapes, indices and counts 4-byte and scratch 16-byte aligned"
                                               : "cotr_depth_corrs: ptrs and cams must be 8-byte, shapes and counts 4-byte, rows and scratch 16-byte aligned");
  if (!scratch || scratch_bytes < scratch_for(n, max_src))
    return handleless_fail(COTR_ERR_ARG, "scratch is NULL or smaller than cotr_depth_corrs_scratch(n, max_src)");
  const int nb = nb_for(max_src);
  unsigned long long* ballots = static_cast<unsigned long long*>(scratch);
  int32_t* offsets = reinterpret_cast<int32_t*>(ballots + (size_t)n * nb * RP_WAVES);
  const unsigned long long* p = reinterpret_cast<const unsigned long long*>(ptrs);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(reproj_flags_kernel<VALID>, dim3(nb, n), dim3(RP_THREADS), 0, s, p, shapes, cams, max_src, nb, ballots);
  hipLaunchKernelGGL(reproj_scan_kernel, dim3(n), dim3(RP_THREADS), 0, s, p, shapes, max_src, nb, ballots, offsets, counts);
  if (cap > 0)
    hipLaunchKernelGGL(reproj_scatter_kernel<VALID>, dim3(nb, n), dim3(RP_THREADS), 0, s, p, shapes, cams, max_src, nb, ballots, offsets,
                       out, cap);
  return launched();
}

}  // namespace

extern "C" {

size_t cotr_depth_corrs_scratch(int n, int max_src) {
  return n > 0 && n <= MAX_ITEMS && max_src > 0 && max_src <= MAX_PIXELS ? scratch_for(n, max_src) : 0;
}

int cotr_depth_corrs(const uint64_t* ptrs, const int32_t* shapes, const double* cams, int n, int max_src, double* rows, int cap,
                     int32_t* counts, void* scratch, size_t scratch_bytes, cotr_stream stream) {
  return compact<false>(ptrs, shapes, cams, n, max_src, rows, cap, counts, scratch, scratch_bytes, stream);
}

int cotr_depth_valid(const uint64_t* ptrs, const int32_t* shapes, int n, int max_src, int32_t* indices, int cap, int32_t* counts,
                     void* scratch, size_t scratch_bytes, cotr_stream stream) {
  return compact<true>(ptrs, shapes, nullptr, n, max_src, indices, cap, counts, scratch, scratch_bytes, stream);
}

int cotr_crop_depth_nearest(const uint64_t* srcs, const int32_t* shapes, const int32_t* boxes, int n, float* dst, int out,
                            cotr_stream stream) {
  if (n < 0 || n > MAX_ITEMS) return handleless_fail(COTR_ERR_ARG, "n must be in [0, 65535]");
  if (n == 0) return COTR_OK;
  if (out < 1 || out > CROP_MAX_OUT) return handleless_fail(COTR_ERR_ARG, "out must be in [1, 4096]");
  if (!srcs || !shapes || !boxes || !dst) return handleless_fail(COTR_ERR_ARG, "srcs, shapes, boxes and dst must not be NULL");
  if (!aligned(srcs, 8)) return handleless_fail(COTR_ERR_ARG, "srcs must be 8-byte aligned");
  hipLaunchKernelGGL(crop_depth_nearest_kernel, dim3((out + CROP_ROWS - 1) / CROP_ROWS, n), dim3(RP_THREADS), (out + CROP_ROWS) * sizeof(int),
                     static_cast<hipStream_t>(stream), reinterpret_cast<const unsigned long long*>(srcs), shapes, boxes, dst, out);
  return launched();
}

}  // extern "C"
