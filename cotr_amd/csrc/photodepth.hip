// Photometric plane-sweep refinement of a depth map: cotr_photo_depth sweeps a few depth hypotheses around the
// depth a reference pixel came with and keeps the one at which the patches of 1 to 31 posed neighbour images look most like the
// reference's (zero-mean normalised cross-correlation over a fronto-parallel patch).  Handle-less (handleless.h), stream-ordered,
// no scratch, integer atomics only, every sum of a pixel made by one thread in one order: the same input gives the same bits.
// Compiled with -ffp-contract=off.
//   1. hl_begin_kernel   (handleless.h) info = {found, 0, ...}
//   2. pd_sweep_kernel   a workgroup per tile of 16 x 16 pixels, a thread per pixel, every sweep of a pixel inside its thread.  In
//                        LDS: the view table (tv_view_row of view_table.h, as md_depth_kernel builds it), the reference tile with
//                        its halo of R pixels ((16 + 2 R)^2 bytes, read for Sa, Saa and every Sab) and the reference ray of every
//                        pixel of that tile (tv_view_ray is two divisions; a tap's ray is its pixel's ray, shared by the (2 R + 1)^2
//                        threads that tap it).  The neighbour samples are byte gathers from global memory: adjacent pixels hit
//                        adjacent bytes.  Nothing per hypothesis stays in registers but the running best and its two neighbours.
// The counters are wave ballots, summed per workgroup in LDS, one integer atomic a counter and workgroup.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "handleless.h"
#define TV_NO_PREPARE_KERNEL   // the table is built in LDS by every workgroup: tv_view_row alone
#include "view_table.h"

using namespace cotr_detail;

#define PD_TILE 16
#define PD_THREADS (PD_TILE * PD_TILE)
#define PD_WAVES (PD_THREADS / 64)
#define PD_MAX_RADIUS 4
#define PD_MAX_STEPS 16
#define PD_MAX_SWEEPS 8
#define PD_SPAN (PD_TILE + 2 * PD_MAX_RADIUS)   // the widest tile with its halo
#define PD_COUNTERS 7

struct PdImage {
  const uint8_t* __restrict__ grey;
  int H, W;
};

// the bilinear sample of view j's image at (u, v), which lies inside it
__device__ __forceinline__ double pd_sample(const PdImage& im, int j, double u, double v) {
  const int x0 = max(min((int)floor(u), im.W - 2), 0), y0 = max(min((int)floor(v), im.H - 2), 0);
  const int x1 = min(x0 + 1, im.W - 1), y1 = min(y0 + 1, im.H - 1);
  const double au = u - (double)x0, av = v - (double)y0;
  const uint8_t* g = im.grey + (size_t)j * ((size_t)im.H * im.W);
  const uint8_t* r0 = g + (size_t)y0 * im.W;
  const uint8_t* r1 = g + (size_t)y1 * im.W;
  const double b0 = (1.0 - au) * (double)r0[x0] + au * (double)r0[x1];
  const double b1 = (1.0 - au) * (double)r1[x0] + au * (double)r1[x1];
  return (1.0 - av) * b0 + av * b1;
}

// what the pixel's thread knows of its patch
struct PdPatch {
  const double* tab;      // the view table in LDS
  const uint8_t* tile;    // the reference tile in LDS, at the patch's first tap
  const double* rays;     // the rays of the tile in LDS, at the patch's first tap
  int span, R;            // a row of the tile, the radius
  double N, Sa, var_a;    // (2 R + 1)^2, the sum of the reference taps, Saa - Sa Sa / N
};

// Whether neighbour j scores at the hypothesis s, and its score there
__device__ bool pd_view_score(const PdPatch& c, const PdImage& im, int j, double s, double min_var_n, double* score) {
  const double* w = c.tab + j * TV_ROW;
  const double* c0 = c.tab + TV_C;
  const TvPixel origin = {0.0, 0.0, true};   // residuals against (0, 0) are the pixel itself
  const double wmax = (double)(im.W - 1), hmax = (double)(im.H - 1);
  const int side = 2 * c.R + 1;
  double Sb = 0.0, Sbb = 0.0, Sab = 0.0;
  for (int dy = 0; dy < side; ++dy)
    for (int dx = 0; dx < side; ++dx) {
      const int at = dy * c.span + dx;
      const double* r = c.rays + at * 3;
      const double X[3] = {c0[0] + s * r[0], c0[1] + s * r[1], c0[2] + s * r[2]};
      const TvProj pr = tv_project(w, origin, X);
      if (!(pr.z > 0.0 && pr.du >= 0.0 && pr.du <= wmax && pr.dv >= 0.0 && pr.dv <= hmax)) return false;   // NaN too
      const double a = (double)c.tile[at], b = pd_sample(im, j, pr.du, pr.dv);
      Sb += b, Sbb += b * b, Sab += a * b;
    }
  const double var_b = Sbb - Sb * Sb / c.N;
  if (!(var_b >= min_var_n)) return false;
  *score = (Sab - c.Sa * Sb / c.N) / sqrt(c.var_a * var_b);
  return true;
}

// per-wavefront counts -> part[wave][col]; then, after a barrier, one atomic a column whose sum is not 0
__device__ __forceinline__ void pd_flush(int (*part)[PD_COUNTERS], const int* mine, int32_t* __restrict__ dst) {
  if ((threadIdx.x & 63) == 0)
    for (int i = 0; i < PD_COUNTERS; ++i) part[threadIdx.x >> 6][i] = mine[i];
  __syncthreads();
  if (threadIdx.x < PD_COUNTERS) {
    int s = 0;
#pragma unroll
    for (int k = 0; k < PD_WAVES; ++k) s += part[k][threadIdx.x];
    if (s) atomicAdd(dst + threadIdx.x, s);
  }
}

__global__ __launch_bounds__(PD_THREADS) void pd_sweep_kernel(const uint8_t* __restrict__ grey, const float* __restrict__ depth_in,
                                                              const double* __restrict__ cams, const double* __restrict__ poses, int V, int H,
                                                              int W, const int32_t* __restrict__ found, int R, int S, int sweeps,
                                                              double rel_step, double min_var, double min_score, int min_views, double dist,
                                                              int keep_input, float* __restrict__ depth_out, float* __restrict__ score_out,
                                                              uint8_t* __restrict__ views_out, int32_t* __restrict__ info) {
  __shared__ double tab[TV_MAX_VIEWS * TV_ROW];
  __shared__ double rays[PD_SPAN * PD_SPAN * 3];
  __shared__ uint8_t tile[PD_SPAN * PD_SPAN];
  __shared__ int part[PD_WAVES][PD_COUNTERS];
  if ((int)threadIdx.x < V) tv_view_row(cams, poses, threadIdx.x, tab + threadIdx.x * TV_ROW);
  __syncthreads();
  const int tx = threadIdx.x % PD_TILE, ty = threadIdx.x / PD_TILE;
  const int tiles_x = (W + PD_TILE - 1) / PD_TILE;   // the tiles row by row in the grid's x: its y would not hold the rows of a tall map
  const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * PD_TILE, y0 = (int)(blockIdx.x / (unsigned)tiles_x) * PD_TILE;
  const int x = x0 + tx, y = y0 + ty;
  const bool in = x < W && y < H;
  const size_t p = (size_t)y * W + x;   // used only where `in`
  const bool on = (found ? found[0] != 0 : true) && tab[TV_OK] != 0.0;   // uniform
  if (!on) {
    if (in) depth_out[p] = 0.0f, score_out[p] = __builtin_nanf(""), views_out[p] = 0;
    return;
  }

  // the reference tile with its halo (0 outside the image: such a tap belongs to rim pixels only) and the ray of each of its pixels
  const int span = PD_TILE + 2 * R;
  for (int i = threadIdx.x; i < span * span; i += PD_THREADS) {
    const int gx = x0 - R + i % span, gy = y0 - R + i / span;
    tile[i] = gx >= 0 && gx < W && gy >= 0 && gy < H ? grey[(size_t)gy * W + gx] : (uint8_t)0;
    tv_view_ray(tab, (double)gx, (double)gy, rays + i * 3);
  }
  __syncthreads();

  // what: 0 refined, 1 no input depth, 2 rim, 3 flat, 4 no hypothesis scored, 5 below min_score, 6 dropped by range; -1 past the map
  int what = -1;
  if (in) {
    const float d_in = depth_in[p];
    float depth = 0.0f, score = __builtin_nanf("");
    int nviews = 0;
    const int side = 2 * R + 1;
    PdPatch c = {tab, tile + ty * span + tx, rays + (ty * span + tx) * 3, span, R, (double)(side * side), 0.0, 0.0};
    const PdImage im = {grey, H, W};
    if (!(d_in > 0.0f && d_in < INFINITY)) {
      what = 1;
    } else if (x < R || y < R || x >= W - R || y >= H - R) {
      what = 2;
    } else {
      double Saa = 0.0;
      for (int dy = 0; dy < side; ++dy)
        for (int dx = 0; dx < side; ++dx) {
          const double a = (double)c.tile[dy * span + dx];
          c.Sa += a, Saa += a * a;
        }
      c.var_a = Saa - c.Sa * c.Sa / c.N;
      const double min_var_n = min_var * c.N;
      if (c.var_a < min_var_n) {
        what = 3;
      } else {
        double centre = (double)d_in, h = rel_step, f_best = 0.0;
        bool have = false;
        int n_best = 0;
        for (int i = 0; i < sweeps; ++i, h *= 0.5) {
          // the running best k, f(k), its views, and f(k - 1), f(k + 1) where they exist
          int k_best = 0;
          double f_minus = 0.0, f_plus = 0.0, f_prev = 0.0;
          bool has_minus = false, has_plus = false, has_prev = false;
          have = false;
          for (int k = -S; k <= S; ++k) {
            const double s = centre * (1.0 + (double)k * h);
            double sum = 0.0;
            int n = 0;
            for (int j = 1; j < V; ++j) {
              if (tab[j * TV_ROW + TV_OK] == 0.0) continue;   // uniform
              double sc;
              if (pd_view_score(c, im, j, s, min_var_n, &sc)) sum += sc, ++n;
            }
            const bool exists = n >= min_views;
            const double f = sum / (double)n;
            if (exists) {
              if (have && k == k_best + 1) f_plus = f, has_plus = true;
              if (!have || f > f_best || (f == f_best && abs(k) < abs(k_best))) {
                have = true, f_best = f, k_best = k, n_best = n;
                f_minus = f_prev, has_minus = has_prev, has_plus = false;
              }
            }
            f_prev = f, has_prev = exists;
          }
          if (have) {
            double delta = 0.0;
            if (abs(k_best) < S && has_minus && has_plus) {
              const double den = (f_minus - 2.0 * f_best) + f_plus;
              if (den < 0.0) delta = fmin(fmax(0.5 * (f_minus - f_plus) / den, -0.5), 0.5);
            }
            centre = centre * (1.0 + ((double)k_best + delta) * h);
          }
        }
        const float d = (float)centre;
        what = !have ? 4 : !(f_best >= min_score) ? 5 : !(d > 0.0f && (double)d < dist) ? 6 : 0;
        if (what == 0) depth = d, score = (float)f_best, nviews = n_best;
      }
    }
    if (what > 1 && keep_input) depth = d_in;
    depth_out[p] = depth, score_out[p] = score, views_out[p] = (uint8_t)nviews;
  }

  int mine[PD_COUNTERS];
#pragma unroll
  for (int i = 0; i < PD_COUNTERS; ++i) mine[i] = __popcll(__ballot(what == i));
  pd_flush(part, mine, info + 1);   // info[1..7]: the seven verdicts
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
namespace {

// do [a, a + na) and [b, b + nb) share a byte (a NULL range shares none)
bool pd_overlap(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b) return false;
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

struct PdRange {
  const void* p;
  size_t bytes;
};

bool pd_finite(double v) { return v > -INFINITY && v < INFINITY; }

}  // namespace

extern "C" {

int cotr_photo_depth(const uint8_t* grey, const float* depth_in, const double* cams, const double* poses, int V, int H, int W,
                     const int32_t* found, int radius, int steps, int sweeps, double rel_step, double min_var, double min_score,
                     int min_views, double distance_thresh, int keep_input, float* depth_out, float* score_out, uint8_t* views_out,
                     int32_t* info_out, cotr_stream stream) {
  static const char* fn = "cotr_photo_depth";
  if (V < 2 || V > TV_MAX_VIEWS) return arg_fail(fn, "V must be in [2, 32]");
  if (H < 1 || W < 1 || (long long)H * W > MAX_PIXELS) return arg_fail(fn, "H and W must be >= 1 with at most 2^28 pixels");
  if (radius < 1 || radius > PD_MAX_RADIUS) return arg_fail(fn, "radius must be in [1, 4]");
  if (steps < 1 || steps > PD_MAX_STEPS) return arg_fail(fn, "steps must be in [1, 16]");
  if (sweeps < 1 || sweeps > PD_MAX_SWEEPS) return arg_fail(fn, "sweeps must be in [1, 8]");
  if (!(rel_step > 0.0) || !pd_finite(rel_step) || !((double)steps * rel_step < 1.0))
    return arg_fail(fn, "rel_step must be finite and > 0 with steps * rel_step < 1");
  if (!(min_var > 0.0) || !pd_finite(min_var)) return arg_fail(fn, "min_var must be finite and > 0");
  if (!(min_score >= -1.0) || !(min_score <= 1.0)) return arg_fail(fn, "min_score must be in [-1, 1]");
  if (min_views < 1 || min_views > V - 1) return arg_fail(fn, "min_views must be in [1, V - 1]");
  if (!(distance_thresh > 0.0) || !pd_finite(distance_thresh)) return arg_fail(fn, "distance_thresh must be finite and > 0");
  if (keep_input != 0 && keep_input != 1) return arg_fail(fn, "keep_input must be 0 or 1");
  if (!grey || !depth_in || !cams || !poses || !depth_out || !score_out || !views_out || !info_out)
    return arg_fail(fn, "grey, depth_in, cams, poses, depth_out, score_out, views_out and info_out must not be NULL");
  if (!aligned(cams, 8) || !aligned(poses, 8) || !aligned(depth_in, 4) || !aligned(depth_out, 4) || !aligned(score_out, 4) ||
      !aligned(info_out, 4) || !aligned(found, 4))
    return arg_fail(fn, "the doubles must be 8-byte, float32 and int32 arrays 4-byte aligned");
  const size_t HW = (size_t)H * W;
  const PdRange r[] = {{depth_out, HW * 4}, {score_out, HW * 4}, {views_out, HW}, {info_out, 32}, {grey, (size_t)V * HW},
                       {depth_in, HW * 4}, {cams, (size_t)V * 40}, {poses, (size_t)V * 96}, {found, 4}};
  for (int a = 0; a < 4; ++a)   // the first four ranges are written
    for (int b = a + 1; b < 9; ++b)
      if (pd_overlap(r[a].p, r[a].bytes, r[b].p, r[b].bytes))
        return arg_fail(fn, "an output must not overlap another output or an input (depth_out is not depth_in)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(hl_begin_kernel<>, dim3(1), dim3(64), 0, s, found, 1, 8, info_out);
  const size_t tiles = (size_t)((W + PD_TILE - 1) / PD_TILE) * (size_t)((H + PD_TILE - 1) / PD_TILE);   // at most 2^28
  hipLaunchKernelGGL(pd_sweep_kernel, dim3((unsigned)tiles), dim3(PD_THREADS), 0, s, grey, depth_in, cams, poses, V, H, W, found, radius, steps, sweeps,
                     rel_step, min_var, min_score, min_views, distance_thresh, keep_input, depth_out, score_out, views_out, info_out);
  return launched();
}

}  // extern "C"
