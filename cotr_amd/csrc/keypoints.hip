// Keypoints of 8-bit grey images: cotr_detect_keypoints, a corner score (min_eig or harris) on the integer structure tensor,
// non-maximum suppression under a total order and the best K by rank.  Handle-less (handleless.h),
// stream-ordered, three launches whatever the data, integer atomics only: the same input gives the same bits, whatever order
// the workgroups ran in.  No gradient, tensor or score map is written to memory: the image is read once, the candidates are
// the only global traffic of the hot path.
//
//   kp_fill_kernel    a thread per output row: NaN / NaN / -1; the counters, the largest keys and info zeroed
//   kp_detect_kernel  a workgroup per 32 x 32 tile of one image: the tile and its halo into LDS once, Sobel, separable box sums,
//                     keys, the candidate test over the (2R+1)^2 window, sub-pixel positions; candidates appended to the
//                     image's list (one atomicAdd per wavefront), the largest key by a 64-bit atomicMax
//   kp_rank_kernel    a thread per candidate: the quality test against the largest key, its rank among the survivors by counting
//                     over LDS tiles of the list, row `rank` written when rank < K; info
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "handleless.h"

using namespace cotr_detail;

#define KP_THREADS 256
#define KP_TILE 32
#define KP_MAX_IMAGES 64
#define KP_MAX_WINDOW 4
#define KP_MAX_NMS 8
#define KP_MAX_K 65536
#define KP_MAX_SIDE (1 << 20)

// Integer bounds (r <= 4): |Ix|, |Iy| <= 4 * 255 = 1020, so a Sobel pair packs into two int16 and a, |b|, c <= 81 * 1020^2 =
// 84 272 400 < 2^31: the box sums are int32 in LDS.  In int64: (a - c)^2 + 4 b b <= 5 * 7.2e15 < 2^56, 64 (a c - b b) <= 4.6e17 and
// 3 (a + c)^2 <= 8.6e16, all far inside 2^63.

// work_out: candidate keys [n][cap] int64 | candidate positions [n][cap][2] float64 | candidate pixels [n][cap] int32 |
// candidates per image [n] int32 | the largest key per image [n] uint64; cap = ceil(H / (R+1)) * ceil(W / (R+1))
struct KpWork {
  long long* key;
  double* xy;
  int32_t* pix;
  int32_t* cnt;
  unsigned long long* top;
  int cap;
  size_t bytes;
};

static KpWork kp_layout(void* base, int n, int H, int W, int R) {
  KpWork l;
  l.cap = ((H + R) / (R + 1)) * ((W + R) / (R + 1));
  const size_t all = (size_t)n * l.cap;
  Carver c(base);
  l.key = c.take<long long>(all);
  l.xy = c.take<double>(2 * all);
  l.pix = c.take<int32_t>(all);
  l.cnt = c.take<int32_t>(n);
  l.top = c.take<unsigned long long>(n);
  l.bytes = c.bytes;
  return l;
}

// the tile's regions in LDS, in bytes: A holds the pixels and the packed gradients, and later the keys; B the three row sums.
// Dynamic LDS of kp_detect_kernel, sized by (r, R); 40 VGPRs, 80 SGPRs, no scratch, so LDS alone bounds the occupancy (160 KiB a CU,
// workgroups of 4 wavefronts):
//   r = 1, R = 1:  9248 + 14688 = 23936 bytes, 6 workgroups = 24 wavefronts a CU
//   r = 2, R = 4 (the defaults): 12800 + 21120 = 33920 bytes, 4 workgroups = 16 wavefronts a CU
//   r = 4, R = 8: 18432 + 32256 = 50688 bytes, 3 workgroups = 12 wavefronts a CU
// Every LDS access of the tile stage is linear in the thread index (32-bit row sums, 64-bit keys, bytes that share a word), so
// the 64 lanes of a wavefront meet no bank twice in a pass; the window scan reads keys at a lane-linear address plus a common
// offset.  kp_rank_kernel: 31 VGPRs, 3328 bytes of static LDS, whose reads are broadcasts; kp_fill_kernel: 10 VGPRs, no LDS.
struct KpLds {
  int PW, GW, KW;   // widths of the pixel tile (halo R + r + 1), the gradient tile (halo R + r) and the key tile (halo R)
  int grad_off, b_off, bytes;
};

static __host__ __device__ __forceinline__ KpLds kp_lds(int r, int R) {
  KpLds s;
  s.PW = KP_TILE + 2 * (R + r + 1), s.GW = s.PW - 2, s.KW = KP_TILE + 2 * R;
  s.grad_off = (s.PW * s.PW + 7) & ~7;
  const int a_px = s.grad_off + s.GW * s.GW * 4, a_key = s.KW * s.KW * 8;
  s.b_off = ((a_px > a_key ? a_px : a_key) + 15) & ~15;
  s.bytes = s.b_off + 3 * s.GW * s.KW * 4;
  return s;
}

// the score a key stands for: harris keys are the score, min_eig keys its bit pattern; key 0 is score 0 in both
__device__ __forceinline__ double kp_score(long long key, int harris) { return harris ? (double)key : __longlong_as_double(key); }

__device__ __forceinline__ double kp_offset(double sm, double s0, double sp) {
  const double den = (sm - s0) + (sp - s0);
  double off = den < 0.0 ? 0.5 * (sm - sp) / den : 0.0;
  off = off < -0.5 ? -0.5 : off;
  return off > 0.5 ? 0.5 : off;
}

__global__ __launch_bounds__(KP_THREADS) void kp_fill_kernel(int n, int K, double* __restrict__ xy_out, double* __restrict__ score_out,
                                                             int32_t* __restrict__ pixel_out, int32_t* __restrict__ info,
                                                             int32_t* __restrict__ cnt, unsigned long long* __restrict__ top) {
  const int i = blockIdx.x * KP_THREADS + threadIdx.x;
  if (i < n) cnt[i] = 0, top[i] = 0ull;
  if (i < 4 * n) info[i] = 0;
  if (i >= n * K) return;
  xy_out[2 * (size_t)i] = NAN, xy_out[2 * (size_t)i + 1] = NAN, score_out[i] = NAN, pixel_out[i] = -1;
}

__global__ __launch_bounds__(KP_THREADS) void kp_detect_kernel(const uint8_t* __restrict__ images, const uint8_t* __restrict__ mask, int H, int W,
                                                               int harris, int r, int R, int margin, double min_score, int cap,
                                                               long long* __restrict__ cand_key, double* __restrict__ cand_xy,
                                                               int32_t* __restrict__ cand_pix, int32_t* __restrict__ cnt,
                                                               unsigned long long* __restrict__ top) {
  extern __shared__ __attribute__((aligned(16))) unsigned char kp_smem[];
  const KpLds s = kp_lds(r, R);
  uint8_t* px = kp_smem;
  int32_t* grad = reinterpret_cast<int32_t*>(kp_smem + s.grad_off);
  long long* keys = reinterpret_cast<long long*>(kp_smem);   // over px and grad, once both are dead
  int32_t* ra = reinterpret_cast<int32_t*>(kp_smem + s.b_off);
  int32_t* rb = ra + s.GW * s.KW;
  int32_t* rc = rb + s.GW * s.KW;
  const int img = blockIdx.z, x0 = blockIdx.x * KP_TILE, y0 = blockIdx.y * KP_TILE, tid = threadIdx.x;
  const uint8_t* im = images + (size_t)img * H * W;
  const uint8_t* mk = mask ? mask + (size_t)img * H * W : nullptr;

  // 1. the pixels, 0 outside the image (a key whose support leaves the image is 0 by the margin, whatever stands there)
  const int h = R + r + 1;
  for (int i = tid; i < s.PW * s.PW; i += KP_THREADS) {
    const int py = i / s.PW, gx = x0 - h + (i - py * s.PW), gy = y0 - h + py;
    px[i] = gx >= 0 && gx < W && gy >= 0 && gy < H ? im[(size_t)gy * W + gx] : 0;
  }
  __syncthreads();
  // 2. Sobel 1-2-1: Ix = right - left, Iy = below - above, packed as two int16
  for (int i = tid; i < s.GW * s.GW; i += KP_THREADS) {
    const int gy = i / s.GW, gx = i - gy * s.GW;
    const uint8_t* p = px + (gy + 1) * s.PW + gx + 1;
    const int a00 = p[-s.PW - 1], a01 = p[-s.PW], a02 = p[-s.PW + 1], a10 = p[-1], a12 = p[1], a20 = p[s.PW - 1], a21 = p[s.PW], a22 = p[s.PW + 1];
    const int ix = (a02 + 2 * a12 + a22) - (a00 + 2 * a10 + a20), iy = (a20 + 2 * a21 + a22) - (a00 + 2 * a01 + a02);
    grad[i] = (ix & 0xffff) | (int)((unsigned)iy << 16);
  }
  __syncthreads();
  // 3. the row pass of the box sums: key column x is gradient column x + r
  for (int i = tid; i < s.GW * s.KW; i += KP_THREADS) {
    const int gy = i / s.KW, kx = i - gy * s.KW;
    const int32_t* g = grad + gy * s.GW + kx;
    int sa = 0, sb = 0, sc = 0;
    for (int d = 0; d <= 2 * r; ++d) {
      const int v = g[d], ix = (int)(short)(v & 0xffff), iy = v >> 16;
      sa += ix * ix, sb += ix * iy, sc += iy * iy;
    }
    ra[i] = sa, rb[i] = sb, rc[i] = sc;
  }
  __syncthreads();
  // 4. the column pass and the keys (written over the pixels and gradients, which nothing reads any more)
  for (int i = tid; i < s.KW * s.KW; i += KP_THREADS) {
    const int ky = i / s.KW, kx = i - ky * s.KW, gx = x0 - R + kx, gy = y0 - R + ky;
    long long key = 0;
    if (gx >= margin && gx < W - margin && gy >= margin && gy < H - margin && (!mk || mk[(size_t)gy * W + gx] != 0)) {
      long long a = 0, b = 0, c = 0;
      for (int d = 0; d <= 2 * r; ++d) a += ra[i + d * s.KW], b += rb[i + d * s.KW], c += rc[i + d * s.KW];
      if (harris) {
        key = 64 * (a * c - b * b) - 3 * (a + c) * (a + c);
      } else {
        const double S = (double)(a + c) - sqrt((double)((a - c) * (a - c) + 4 * b * b));
        key = S > 0.0 ? __double_as_longlong(S) : 0;
      }
      key = key > 0 ? key : 0;
    }
    keys[i] = key;
  }
  __syncthreads();
  // 5. candidates of the tile's own 32 x 32 pixels; every thread runs every round, so the ballots see whole wavefronts
  const int lane = tid & 63;
  for (int round = 0; round < KP_TILE * KP_TILE / KP_THREADS; ++round) {
    const int i = round * KP_THREADS + tid, ty = i / KP_TILE, tx = i - ty * KP_TILE, gx = x0 + tx, gy = y0 + ty;
    const long long* kc = keys + (ty + R) * s.KW + tx + R;
    const long long key = gx < W && gy < H ? *kc : 0;
    bool cand = key > 0 && kp_score(key, harris) >= min_score;
    for (int dy = -R; cand && dy <= R; ++dy)
      for (int dx = -R; dx <= R; ++dx) {
        const long long q = kc[dy * s.KW + dx];
        // a pixel before p in raster order must be smaller, one behind it may be equal
        if (dy < 0 || (dy == 0 && dx < 0) ? q >= key : q > key) {
          cand = false;
          break;
        }
      }
    const unsigned long long votes = __ballot(cand);
    if (votes == 0ull) continue;   // the whole wavefront
    int base = 0;
    if (lane == 0) base = atomicAdd(cnt + img, __popcll(votes));
    base = __shfl(base, 0, 64);
    unsigned long long best = cand ? (unsigned long long)key : 0ull;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long o = __shfl_xor(best, off, 64);
      best = o > best ? o : best;
    }
    if (lane == 0) atomicMax(top + img, best);
    const int slot = base + __popcll(votes & ((1ull << lane) - 1ull));
    if (cand && slot < cap) {   // slot < cap always: no two candidates lie within R of each other
      const double s0 = kp_score(key, harris);
      const size_t at = (size_t)img * cap + slot;
      cand_key[at] = key, cand_pix[at] = gy * W + gx;
      cand_xy[2 * at] = (double)gx + kp_offset(kp_score(kc[-1], harris), s0, kp_score(kc[1], harris));
      cand_xy[2 * at + 1] = (double)gy + kp_offset(kp_score(kc[-s.KW], harris), s0, kp_score(kc[s.KW], harris));
    }
  }
}

__device__ __forceinline__ int kp_wave_sum(int a) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a = a + __shfl_xor(a, off);
  return a;
}

// The rank of a survivor is the number of survivors ahead of it in the total order (key descending, pixel ascending): counted,
// not sorted, so it does not depend on where the appends put anything.  A candidate that fails the quality test enters the
// tiles as key 0, which is ahead of nothing.
__global__ __launch_bounds__(KP_THREADS) void kp_rank_kernel(int harris, double quality, int K, int cap, const long long* __restrict__ cand_key,
                                                             const double* __restrict__ cand_xy, const int32_t* __restrict__ cand_pix,
                                                             const int32_t* __restrict__ cnt, const unsigned long long* __restrict__ top,
                                                             double* __restrict__ xy_out, double* __restrict__ score_out,
                                                             int32_t* __restrict__ pixel_out, int32_t* __restrict__ info) {
  __shared__ long long tkey[KP_THREADS];
  __shared__ int tpix[KP_THREADS];
  const int img = blockIdx.y, tid = threadIdx.x;
  int M = cnt[img];
  M = M < cap ? M : cap;
  if ((int)blockIdx.x * KP_THREADS >= M) return;   // the whole workgroup
  const double floor_s = quality * kp_score((long long)top[img], harris);
  const long long* ck = cand_key + (size_t)img * cap;
  const int32_t* cp = cand_pix + (size_t)img * cap;
  const int i = blockIdx.x * KP_THREADS + tid;
  long long key = 0;
  int pix = 0;
  if (i < M) {
    key = ck[i], pix = cp[i];
    if (!(kp_score(key, harris) >= floor_s)) key = 0;
  }
  if (i == 0) info[4 * img] = M;
  // a workgroup none of whose candidates passed the quality test has nothing to rank: where quality cuts most of the list,
  // the counting is bounded by the workgroups that hold a survivor
  if (!__syncthreads_or(key > 0 ? 1 : 0)) return;
  int ahead = 0;
  for (int base = 0; base < M; base += KP_THREADS) {
    const int j = base + tid;
    long long kj = 0;
    int pj = 0;
    if (j < M) {
      kj = ck[j], pj = cp[j];
      if (!(kp_score(kj, harris) >= floor_s)) kj = 0;
    }
    tkey[tid] = kj, tpix[tid] = pj;   // past the list's end key 0: ahead of nothing that is alive
    __syncthreads();
    // a fixed trip count, unrolled, so that the LDS reads of a batch are in flight together; the steps are bound by their 64-bit
    // compares all the same
#pragma unroll 16
    for (int t = 0; t < KP_THREADS; ++t) {
      const long long q = tkey[t];
      ahead += (q > key || (q == key && tpix[t] < pix)) ? 1 : 0;
    }
    __syncthreads();
  }
  const bool alive = key > 0, put = alive && ahead < K;
  if (put) {
    const size_t row = (size_t)img * K + ahead, at = (size_t)img * cap + i;
    xy_out[2 * row] = cand_xy[2 * at], xy_out[2 * row + 1] = cand_xy[2 * at + 1];
    score_out[row] = kp_score(key, harris), pixel_out[row] = pix;
  }
  const int na = kp_wave_sum(alive ? 1 : 0), np = kp_wave_sum(put ? 1 : 0);
  if ((tid & 63) == 0) {
    if (na) atomicAdd(info + 4 * img + 1, na);
    if (np) atomicAdd(info + 4 * img + 2, np);
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
namespace {

const char* const KP_FN = "cotr_detect_keypoints";

const char* kp_check_shape(int n, int H, int W, int R) {
  if (n < 1 || n > KP_MAX_IMAGES) return "n must be in [1, 64]";
  if (R < 1 || R > KP_MAX_NMS) return "nms_radius must be in [1, 8]";
  // H, W <= 2^20: the tile grid's y dimension, ceil(H / 32), stays inside what a launch takes
  if (H < 1 || W < 1 || H > KP_MAX_SIDE || W > KP_MAX_SIDE || (long long)n * H * W > MAX_PIXELS)
    return "H, W must be in [1, 2^20] and n * H * W at most 2^28";
  return nullptr;
}

}  // namespace

extern "C" {

int cotr_detect_keypoints_work_bytes(int n, int H, int W, int nms_radius, size_t* bytes) {
  if (!bytes) return arg_fail("cotr_detect_keypoints_work_bytes", "bytes is NULL");
  if (const char* msg = kp_check_shape(n, H, W, nms_radius)) return arg_fail(KP_FN, msg);
  *bytes = kp_layout(nullptr, n, H, W, nms_radius).bytes;
  return COTR_OK;
}

int cotr_detect_keypoints(const uint8_t* images, const uint8_t* mask, int n, int H, int W, int score, int window_radius, int nms_radius,
                          int border, double quality, double min_score, int max_keypoints, double* xy_out, double* score_out,
                          int32_t* pixel_out, int32_t* info_out, void* work_out, cotr_stream stream) {
  const int r = window_radius, R = nms_radius, K = max_keypoints;
  if (const char* msg = kp_check_shape(n, H, W, R)) return arg_fail(KP_FN, msg);
  if (score != 0 && score != 1) return arg_fail(KP_FN, "score must be 0 (min_eig) or 1 (harris)");
  if (r < 1 || r > KP_MAX_WINDOW) return arg_fail(KP_FN, "window_radius must be in [1, 4]");
  if (border < 0) return arg_fail(KP_FN, "border must be >= 0");
  const long long margin = border > r + 1 ? border : r + 1;
  if (2 * margin + 1 > H || 2 * margin + 1 > W) return arg_fail(KP_FN, "H and W must be at least 2 max(border, window_radius + 1) + 1");
  if (!(quality >= 0.0 && quality <= 1.0)) return arg_fail(KP_FN, "quality must be in [0, 1]");
  if (min_score != min_score) return arg_fail(KP_FN, "min_score must not be NaN");
  if (K < 1 || K > KP_MAX_K) return arg_fail(KP_FN, "max_keypoints must be in [1, 65536]");
  if (!images || !xy_out || !score_out || !pixel_out || !info_out || !work_out)
    return arg_fail(KP_FN, "images, xy_out, score_out, pixel_out, info_out and work_out must not be NULL");
  if (!aligned(xy_out, 8) || !aligned(score_out, 8) || !aligned(work_out, 8) || !aligned(pixel_out, 4) || !aligned(info_out, 4))
    return arg_fail(KP_FN, "doubles and work_out must be 8-byte and ints 4-byte aligned");
  const KpWork l = kp_layout(work_out, n, H, W, R);
  const KpLds s = kp_lds(r, R);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rows = n * K;   // >= 4 n
  const unsigned fill = (unsigned)(((rows > 4 * n ? rows : 4 * n) + KP_THREADS - 1) / KP_THREADS);
  hipLaunchKernelGGL(kp_fill_kernel, dim3(fill), dim3(KP_THREADS), 0, st, n, K, xy_out, score_out, pixel_out, info_out, l.cnt, l.top);
  const dim3 tiles((unsigned)((W + KP_TILE - 1) / KP_TILE), (unsigned)((H + KP_TILE - 1) / KP_TILE), (unsigned)n);
  hipLaunchKernelGGL(kp_detect_kernel, tiles, dim3(KP_THREADS), (size_t)s.bytes, st, images, mask, H, W, score, r, R, (int)margin, min_score, l.cap,
                     l.key, l.xy, l.pix, l.cnt, l.top);
  hipLaunchKernelGGL(kp_rank_kernel, dim3((unsigned)((l.cap + KP_THREADS - 1) / KP_THREADS), (unsigned)n), dim3(KP_THREADS), 0, st, score, quality, K,
                     l.cap, (const long long*)l.key, (const double*)l.xy, (const int32_t*)l.pix, (const int32_t*)l.cnt,
                     (const unsigned long long*)l.top, xy_out, score_out, pixel_out, info_out);
  return launched();
}

}  // extern "C"
