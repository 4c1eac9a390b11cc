// Delaunay triangulation of the correspondences' normalised A points on the device: the step of triangulate_corr that
// scipy.spatial.Delaunay did on the host (COTR/inference/inference_helper.py:239,293-308).  The rule is exact, unique for every
// input and fully specified:
//   - points snapped to 2^-24: X = rint(u * 2^24), Y = rint(v * 2^24) (double, from the float32 input); a point is valid when
//     it is finite, |X|, |Y| <= 2^26 and no valid point of lower index has the same (X, Y); invalid points take no part;
//   - orient(p, q, r) = (q - p) x (r - p), exact in int64; d is inside the circle of the counter-clockwise a, b, c when
//     det0 = |a'|^2 (b' x c') - |b'|^2 (a' x c') + |c'|^2 (a' x b') > 0 (primes: minus d), exact in 128-bit integers behind
//     a double filter whose error bound is Shewchuk's for exact differences, so the decision is always the exact one;
//   - det0 == 0: the sign of the cofactor (C_a = b' x c', C_b = -a' x c', C_c = a' x b', C_d = -orient(a, b, c)) of the
//     lowest point index whose cofactor is not 0 - the regular triangulation of heights raised infinitesimally, more for a
//     lower index;
//   - apex(a, b): among the valid points strictly left of a->b the one no other candidate is inside the circle of; the
//     candidates are totally ordered by that test, so every lane keeps its best and a butterfly reduces the wavefront;
//   - one walk per valid point p, from its nearest valid point q0 (exact squared distance, lowest index on ties)
//     counter-clockwise, c = apex(p, q): (p, q, c), q = c, until c == q0 or there is no c; then, from q0 the other way,
//     c = apex(q, p): (p, c, q), q = c; a triangle is kept by the walk of its lowest index only;
//   - output ordered by p, then in walk order; rows past the count are -1; info = {count, status}, status 1 when a walk
//     reached its bound of n steps (it stops there).
//
//   1. del_snap_kernel    a thread per point: snapping and the range test; info = {0, 0}
//   2. del_dedup_kernel   a wavefront per point: equal snapped points of lower index make it invalid
//   3. del_walk_kernel    a wavefront per point: the walk; the first STAGE kept triangles go to scratch, the number kept to cnt
//   4. del_scan_kernel    one workgroup: the row of every point from cnt (scan.h), the total to info[0]
//   5. del_write_kernel   a wavefront per point: the staged triangles to their rows (a point that kept more than STAGE walks
//                         again and writes directly); rows past the count to -1
// The coordinate array (8 bytes per point, at most 512 KiB) is read by every wavefront in the same order and stays in L2.
// No atomics decide a position, no host waits, no allocation: capturable.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "handleless.h"
#include "scan.h"

using namespace cotr_detail;

#define DEL_MAX_N 65536
#define DEL_THREADS 256
#define DEL_WAVES (DEL_THREADS / 64)
#define DEL_STAGE 8                  // kept triangles per point held in scratch between the walk and the write
#define DEL_INVALID 0x7fffffff       // x of a point that takes no part (valid |X| <= 2^26)
#define DEL_SCALE 16777216.0         // 2^24
#define DEL_LIMIT 67108864.0         // 2^26

typedef __int128 i128;

__device__ __forceinline__ long long orient2(int2 p, int2 q, int2 r) {   // differences < 2^28: every product below 2^56
  return (long long)(q.x - p.x) * (r.y - p.y) - (long long)(q.y - p.y) * (r.x - p.x);
}

// is d inside the circle of the counter-clockwise a, b, c, by the rule above (ia .. id: the point indices, all different)
__device__ bool in_circle(int ia, int2 a, int ib, int2 b, int ic, int2 c, int id, int2 d) {
  const int iax = a.x - d.x, iay = a.y - d.y, ibx = b.x - d.x, iby = b.y - d.y, icx = c.x - d.x, icy = c.y - d.y;
  {
    // the differences are exact in double, so Shewchuk's bound for the expression below holds: (10 + 96 eps) eps * permanent
    const double ax = iax, ay = iay, bx = ibx, by = iby, cx = icx, cy = icy;
    const double bxcy = bx * cy, cxby = cx * by, cxay = cx * ay, axcy = ax * cy, axby = ax * by, bxay = bx * ay;
    const double la = ax * ax + ay * ay, lb = bx * bx + by * by, lc = cx * cx + cy * cy;
    const double det = la * (bxcy - cxby) + lb * (cxay - axcy) + lc * (axby - bxay);
    const double perm = (fabs(bxcy) + fabs(cxby)) * la + (fabs(cxay) + fabs(axcy)) * lb + (fabs(axby) + fabs(bxay)) * lc;
    const double bound = 1.1102230246251577e-15 * perm;   // (10 + 96 * 2^-53) * 2^-53, rounded up
    if (det > bound) return true;
    if (-det > bound) return false;
  }
  const long long ax = iax, ay = iay, bx = ibx, by = iby, cx = icx, cy = icy;
  const long long Ca = bx * cy - by * cx, Cb = -(ax * cy - ay * cx), Cc = ax * by - ay * bx;   // each below 2^57
  const i128 det = (i128)(ax * ax + ay * ay) * Ca + (i128)(bx * bx + by * by) * Cb + (i128)(cx * cx + cy * cy) * Cc;
  if (det != 0) return det > 0;
  const long long Cd = -orient2(a, b, c);   // < 0: a, b, c are counter-clockwise
  int low = id;
  bool in = Cd > 0;
  if (Cc != 0 && ic < low) low = ic, in = Cc > 0;
  if (Cb != 0 && ib < low) low = ib, in = Cb > 0;
  if (Ca != 0 && ia < low) low = ia, in = Ca > 0;
  return in;
}

// apex(a, b); every lane of the wavefront calls it with the same a, b and gets the same answer
__device__ int apex(const int2* __restrict__ pts, int n, int ia, int2 a, int ib, int2 b, int lane) {
  int best = -1;
  int2 c = make_int2(0, 0);
  for (int j = lane; j < n; j += 64) {
    const int2 d = pts[j];
    if (d.x == DEL_INVALID || orient2(a, b, d) <= 0) continue;   // (a and b themselves: orient == 0)
    if (best < 0 || in_circle(ia, a, ib, b, best, c, j, d)) best = j, c = d;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const int o = __shfl_xor(best, m, 64);
    const int2 e = make_int2(__shfl_xor(c.x, m, 64), __shfl_xor(c.y, m, 64));
    if (o < 0 || o == best) continue;
    bool take = best < 0;
    if (!take) take = o > best ? in_circle(ia, a, ib, b, best, c, o, e) : !in_circle(ia, a, ib, b, o, e, best, c);   // both lanes of a pair ask the same question
    if (take) best = o, c = e;
  }
  return __builtin_amdgcn_readfirstlane(best);
}

// the nearest valid point of p (exact squared distance, the lowest index on ties), -1 when p is the only valid point
__device__ int nearest(const int2* __restrict__ pts, int n, int ip, int2 p, int lane) {
  long long bd = 0x7fffffffffffffffLL;
  int best = 0x7fffffff;
  for (int j = lane; j < n; j += 64) {
    const int2 d = pts[j];
    if (d.x == DEL_INVALID || j == ip) continue;
    const long long dx = d.x - p.x, dy = d.y - p.y, dd = dx * dx + dy * dy;
    if (dd < bd) bd = dd, best = j;   // j ascends: a tie keeps the lower index
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const long long od = __shfl_xor(bd, m, 64);
    const int o = __shfl_xor(best, m, 64);
    if (od < bd || (od == bd && o < best)) bd = od, best = o;
  }
  best = __builtin_amdgcn_readfirstlane(best);
  return best == 0x7fffffff ? -1 : best;
}

// the walk of point ip; sink(k, q, c) takes the k-th kept triangle (ip, q, c).  Returns the number kept.
template <class Sink>
__device__ int walk(const int2* __restrict__ pts, int n, int ip, int lane, int* __restrict__ info, Sink sink) {
  const int2 p = pts[ip];
  if (p.x == DEL_INVALID) return 0;
  const int q0 = nearest(pts, n, ip, p, lane);
  if (q0 < 0) return 0;
  int kept = 0, steps = 0, q = q0;
  int2 Q = pts[q];
  bool open = false;
  for (;;) {
    if (steps++ >= n) {   // cannot happen for a consistent rule; the bound keeps a wavefront from spinning if it ever does
      if (lane == 0) atomicOr(&info[1], 1);
      return kept;
    }
    const int c = apex(pts, n, ip, p, q, Q, lane);
    if (c < 0) {
      open = true;
      break;
    }
    if (ip < q && ip < c) sink(kept++, q, c);
    q = c, Q = pts[c];
    if (c == q0) break;
  }
  if (!open) return kept;
  q = q0, Q = pts[q];
  for (;;) {
    if (steps++ >= n) {
      if (lane == 0) atomicOr(&info[1], 1);
      return kept;
    }
    const int c = apex(pts, n, q, Q, ip, p, lane);
    if (c < 0) break;
    if (ip < q && ip < c) sink(kept++, c, q);
    q = c, Q = pts[c];
  }
  return kept;
}

__global__ __launch_bounds__(DEL_THREADS) void del_snap_kernel(const float* __restrict__ verts, int n, int2* __restrict__ raw,
                                                               int* __restrict__ info) {
  const int i = blockIdx.x * DEL_THREADS + threadIdx.x;
  if (i == 0) info[0] = 0, info[1] = 0;
  if (i >= n) return;
  const double x = rint((double)verts[(size_t)i * 2] * DEL_SCALE), y = rint((double)verts[(size_t)i * 2 + 1] * DEL_SCALE);
  const bool ok = fabs(x) <= DEL_LIMIT && fabs(y) <= DEL_LIMIT;   // false for NaN and inf as well
  raw[i] = ok ? make_int2((int)x, (int)y) : make_int2(DEL_INVALID, 0);
}

__global__ __launch_bounds__(DEL_THREADS) void del_dedup_kernel(const int2* __restrict__ raw, int n, int2* __restrict__ pts) {
  const int lane = threadIdx.x & 63;
  const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * DEL_WAVES + (threadIdx.x >> 6));
  if (i >= n) return;
  const int2 p = raw[i];
  bool dup = false;
  if (p.x != DEL_INVALID)
    for (int j = lane; j < i; j += 64) {   // the lowest index of equal in-range points is the valid one: any equal j < i decides
      const int2 d = raw[j];
      dup = dup || (d.x == p.x && d.y == p.y);
    }
  const bool any = __any(dup);
  if (lane == 0) pts[i] = any ? make_int2(DEL_INVALID, 0) : p;
}

__global__ __launch_bounds__(DEL_THREADS) void del_walk_kernel(const int2* __restrict__ pts, int n, int2* __restrict__ stage,
                                                               int* __restrict__ cnt, int* __restrict__ info) {
  const int lane = threadIdx.x & 63;
  const int ip = __builtin_amdgcn_readfirstlane(blockIdx.x * DEL_WAVES + (threadIdx.x >> 6));
  if (ip >= n) return;
  int2* mine = stage + (size_t)ip * DEL_STAGE;
  const int kept = walk(pts, n, ip, lane, info, [&](int k, int q, int c) {
    if (lane == 0 && k < DEL_STAGE) mine[k] = make_int2(q, c);
  });
  if (lane == 0) cnt[ip] = kept;
}

// off[i] = cnt[0] + .. + cnt[i - 1]; the total (at most cap) to info[0]
__global__ __launch_bounds__(DEL_THREADS) void del_scan_kernel(const int* __restrict__ cnt, int* __restrict__ off, int n, int cap,
                                                               int* __restrict__ info) {
  __shared__ int sums[DEL_WAVES];
  // a segment of cnt per thread and one scan of the segment sums, not scan_array's walk: at 65536 points that is 256 chunks, each
  // behind the latency of its own load, and it measured 0.2 to 0.4 ms slower
  const int per = (n + DEL_THREADS - 1) / DEL_THREADS;
  const int lo = min((int)threadIdx.x * per, n), hi = min(lo + per, n);
  int sum = 0;
  for (int i = lo; i < hi; ++i) sum += cnt[i];
  int total;
  int run = cotr_scan::block_scan<DEL_WAVES>(sum, sums, &total);
  for (int i = lo; i < hi; ++i) {
    off[i] = run;
    run += cnt[i];
  }
  if (threadIdx.x == 0) info[0] = min(total, cap);
}

__global__ __launch_bounds__(DEL_THREADS) void del_write_kernel(const int2* __restrict__ pts, int n, const int2* __restrict__ stage,
                                                                const int* __restrict__ cnt, const int* __restrict__ off, int cap,
                                                                int32_t* __restrict__ tris, int* __restrict__ info) {
  const int row = blockIdx.x * DEL_THREADS + threadIdx.x;
  if (row < cap && row >= info[0]) tris[(size_t)row * 3] = -1, tris[(size_t)row * 3 + 1] = -1, tris[(size_t)row * 3 + 2] = -1;
  const int lane = threadIdx.x & 63;
  const int ip = __builtin_amdgcn_readfirstlane(blockIdx.x * DEL_WAVES + (threadIdx.x >> 6));
  if (ip >= n) return;
  const int kept = cnt[ip], base = off[ip];
  if (kept <= DEL_STAGE) {
    if (lane < kept && base + lane < cap) {
      const int2 t = stage[(size_t)ip * DEL_STAGE + lane];
      int32_t* r = tris + (size_t)(base + lane) * 3;
      r[0] = ip, r[1] = t.x, r[2] = t.y;
    }
    return;
  }
  walk(pts, n, ip, lane, info, [&](int k, int q, int c) {
    if (lane == 0 && k < kept && base + k < cap) {
      int32_t* r = tris + (size_t)(base + k) * 3;
      r[0] = ip, r[1] = q, r[2] = c;
    }
  });
}

// ---- host side ------------------------------------------------------------------------------------------------------
namespace {

struct Layout {
  int2 *raw, *pts;   // [n] the snapped points, before and after the duplicates left
  int2* stage;       // [n][DEL_STAGE]
  int *cnt, *off;    // [n]
  size_t bytes;
};

Layout layout(void* base, int n) {
  Layout l;
  Carver c(base);
  l.raw = c.take<int2>(n);
  l.pts = c.take<int2>(n);
  l.stage = c.take<int2>((size_t)n * DEL_STAGE);
  l.cnt = c.take<int>(n);
  l.off = c.take<int>(n);
  l.bytes = c.bytes;
  return l;
}

const char* check_n(int n) { return n < 0 || n > DEL_MAX_N ? "n must be in [0, 65536]" : nullptr; }

}  // namespace

extern "C" {

int cotr_delaunay_max_tris(int n) {
  if (check_n(n)) return handleless_fail(COTR_ERR_ARG, "cotr_delaunay_max_tris: n must be in [0, 65536]");
  return 2 * n;
}

int cotr_delaunay_scratch_bytes(int n, size_t* bytes) {
  if (!bytes) return handleless_fail(COTR_ERR_ARG, "cotr_delaunay_scratch_bytes: bytes is NULL");
  if (const char* e = check_n(n)) return handleless_fail(COTR_ERR_ARG, e);
  *bytes = layout(nullptr, n).bytes;
  return COTR_OK;
}

int cotr_delaunay(const float* verts, int n, int32_t* tris, int32_t* info, void* scratch, size_t scratch_bytes, cotr_stream stream) {
  if (const char* e = check_n(n)) return handleless_fail(COTR_ERR_ARG, e);
  if (!info) return handleless_fail(COTR_ERR_ARG, "info must not be NULL");
  if (n > 0 && (!verts || !tris || !scratch)) return handleless_fail(COTR_ERR_ARG, "verts, tris and scratch must not be NULL");
  if (!aligned(scratch, 16) || !aligned(verts, 4) || !aligned(tris, 4) || !aligned(info, 4))
    return handleless_fail(COTR_ERR_ARG, "scratch must be 16-byte, verts, tris and info 4-byte aligned");
  const Layout l = layout(scratch, n);
  if (scratch_bytes < l.bytes) return handleless_fail(COTR_ERR_ARG, "scratch is smaller than cotr_delaunay_scratch_bytes");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int cap = 2 * n;
  hipLaunchKernelGGL(del_snap_kernel, dim3(n > 0 ? (n + DEL_THREADS - 1) / DEL_THREADS : 1), dim3(DEL_THREADS), 0, s, verts, n, l.raw, info);
  if (n > 0) {
    const dim3 waves((n + DEL_WAVES - 1) / DEL_WAVES);   // a wavefront per point; 64 n threads >= the 2 n rows of tris
    hipLaunchKernelGGL(del_dedup_kernel, waves, dim3(DEL_THREADS), 0, s, l.raw, n, l.pts);
    hipLaunchKernelGGL(del_walk_kernel, waves, dim3(DEL_THREADS), 0, s, l.pts, n, l.stage, l.cnt, info);
    hipLaunchKernelGGL(del_scan_kernel, dim3(1), dim3(DEL_THREADS), 0, s, l.cnt, l.off, n, cap, info);
    hipLaunchKernelGGL(del_write_kernel, waves, dim3(DEL_THREADS), 0, s, l.pts, n, l.stage, l.cnt, l.off, cap, tris, info);
  }
  return launched();
}

}  // extern "C"
