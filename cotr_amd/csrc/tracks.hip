// Multi-view tracks from pairwise keypoint matches: cotr_build_tracks, the connected components of the match graph under a
// consistency rule.  Handle-less (handleless.h), stream-ordered, seven launches whatever the data, integer
// arithmetic and integer atomics only: the same input gives the same bits, whatever order the hardware runs the matches in.
// The call takes no scratch: its state lives in work_out, an output the header documents, cut by the Carver of handleless.h.
//
//   tk_init_kernel     a thread per node: its own parent, masks and touched flag cleared; the counters zeroed
//   tk_hook_kernel     a thread per match: dead or live, the touched flags, lock-free union-find by compare-and-swap
//   tk_label_kernel    a thread per node: the walk to its root, the root's view mask, and its conflict mask from the old value
//   tk_flag_kernel     a thread per node: a root decides whether its component is a track; positions within the workgroup, totals
//   tk_scan_kernel     one workgroup: scan_array over the totals; info [0], [1], [3] .. [6], and [2], [7] zeroed
//   tk_fill_kernel     a thread per cell of [V][cap]: empty
//   tk_scatter_kernel  a thread per node: track_of_node, and a written observation into its own cell; info [2], [7]
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "handleless.h"
#include "scan.h"

using namespace cotr_detail;

#define TK_THREADS 256
#define TK_WAVES (TK_THREADS / 64)
#define TK_MAX_VIEWS 32
#define TK_MAX_NODES (1 << 21)
#define TK_MAX_MATCHES (1 << 24)
// counters: live matches | components | components with a view in conflict | components dropped as too short
#define TK_CNT_LIVE 0
#define TK_CNT_COMP 1
#define TK_CNT_CONF 2
#define TK_CNT_SHORT 3
#define TK_COUNTERS 8

// work_out: parents [K] (after tk_flag_kernel: at a root the position of its track within its workgroup, or -1) | labels [K] |
// seen masks [K] | conflict masks [K] | touched flags [K] uint8 | block sums [ceil(K / 256)] | counters [8]
struct TkWork {
  int32_t* parent;
  int32_t* label;
  uint32_t* seen;
  uint32_t* conflict;
  uint8_t* touched;
  int32_t* bsum;
  int32_t* cnt;
  size_t ints;
};

static TkWork tk_layout(int32_t* base, int K, int M) {
  (void)M;   // a thread a match keeps no state of its own
  const size_t N = (size_t)K, blocks = (N + TK_THREADS - 1) / TK_THREADS;
  Carver c(base);
  TkWork l;
  l.parent = c.take<int32_t>(N);
  l.label = c.take<int32_t>(N);
  l.seen = c.take<uint32_t>(N);
  l.conflict = c.take<uint32_t>(N);
  l.touched = c.take<uint8_t>(N);
  l.bsum = c.take<int32_t>(blocks);
  l.cnt = c.take<int32_t>(TK_COUNTERS);
  l.ints = c.bytes / sizeof(int32_t);
  return l;
}

// the V + 1 entries of offsets into LDS (the search reads [1] .. [V - 1], the local index [v]); the caller owes the barrier
__device__ __forceinline__ void tk_load_offsets(int* offs, const int32_t* __restrict__ offsets, int V) {
  if ((int)threadIdx.x <= V) offs[threadIdx.x] = offsets[threadIdx.x];
}

// The view of node g: the largest v in [0, V) with offsets[v] <= g, by a binary search that reads entries 1 .. V - 1 only and so
// stays in [0, V) whatever the table holds (a table that decreases gives some view in range, the same one every time).
__device__ __forceinline__ int tk_view(const int* offs, int V, int g) {
  int lo = 0, hi = V;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offs[mid] <= g)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int tk_wave_sum(int a) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) a = a + __shfl_xor(a, off);
  return a;
}

// every read of parent while hooks are in flight: an agent-scope atomic load (a plain load may be served from a line that
// another XCD's compare-and-swap has since changed)
__device__ __forceinline__ int tk_parent(const int32_t* parent, int x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The walk to the root, halving the path behind it: a node that is no root (parent[x] = p < x, and it never becomes one again)
// is pointed at its grandparent by atomicMin, which only lowers parent[x], to an ancestor in the same set, and leaves roots alone.
// Without it a path of K nodes hooked end to end costs every later walk O(K) loads.
__device__ __forceinline__ int tk_find(int32_t* parent, int x) {
  for (;;) {
    const int p = tk_parent(parent, x);
    if (p == x) return x;
    const int gp = tk_parent(parent, p);
    if (gp != p) atomicMin(parent + x, gp);
    x = p;   // p < x: the walk descends
  }
}

__global__ __launch_bounds__(TK_THREADS) void tk_init_kernel(int K, int32_t* __restrict__ parent, uint32_t* __restrict__ seen,
                                                             uint32_t* __restrict__ conflict, uint8_t* __restrict__ touched,
                                                             int32_t* __restrict__ cnt) {
  const int g = blockIdx.x * TK_THREADS + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < TK_COUNTERS) cnt[threadIdx.x] = 0;
  if (g >= K) return;
  parent[g] = g, seen[g] = 0u, conflict[g] = 0u, touched[g] = 0;
}

// Termination and the labels.  parent[x] <= x holds at the start (parent[x] = x) and every write is a successful
// atomicCAS(&parent[hi], hi, lo) with lo < hi or the atomicMin of tk_find, so it holds always, a node that stopped being a root
// never becomes one again, and a value of parent only ever falls.  Every walk therefore strictly descends and ends at a root.  A compare-and-swap fails only
// because parent[hi] no longer is hi: another thread's hook succeeded since this thread read it.  At most K - 1 hooks succeed in
// the whole launch, so a thread fails finitely often; between failures it walks finitely far; it never waits for another thread.
// A hook joins two roots of different sets under the smaller one, so the root of a set always is its smallest node, and when the
// launch ends the sets are the connected components of the live matches: the root of a node is its component's smallest id,
// whatever order the matches ran in.
__global__ __launch_bounds__(TK_THREADS) void tk_hook_kernel(const int32_t* __restrict__ offsets, const int32_t* __restrict__ matches,
                                                             const uint8_t* __restrict__ keep, int V, int K, int M,
                                                             int32_t* parent, uint8_t* __restrict__ touched, int32_t* __restrict__ cnt) {
  __shared__ int offs[TK_MAX_VIEWS + 1];
  tk_load_offsets(offs, offsets, V);
  __syncthreads();
  const int m = blockIdx.x * TK_THREADS + threadIdx.x;
  bool live = false;
  int a = 0, b = 0;
  if (m < M) {
    a = matches[2 * (size_t)m], b = matches[2 * (size_t)m + 1];
    live = a >= 0 && a < K && b >= 0 && b < K && (!keep || keep[m] != 0);
    live = live && tk_view(offs, V, a) != tk_view(offs, V, b);   // a = b lies in one view
  }
  const int n = tk_wave_sum(live ? 1 : 0);
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(cnt + TK_CNT_LIVE, n);
  if (!live) return;
  touched[a] = 1, touched[b] = 1;   // every writer stores the same byte
  a = tk_find(parent, a), b = tk_find(parent, b);
  while (a != b) {
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) break;
    a = tk_find(parent, old), b = tk_find(parent, lo);   // from the value the compare-and-swap returned: old < hi
  }
}

// after the kernel boundary the sets and their roots are final; the walks go on halving the paths, so parent is still read by
// atomic loads here
__global__ __launch_bounds__(TK_THREADS) void tk_label_kernel(const int32_t* __restrict__ offsets, int V, int K,
                                                              int32_t* parent, const uint8_t* __restrict__ touched,
                                                              int32_t* __restrict__ label, uint32_t* __restrict__ seen,
                                                              uint32_t* __restrict__ conflict) {
  __shared__ int offs[TK_MAX_VIEWS + 1];
  tk_load_offsets(offs, offsets, V);
  __syncthreads();
  const int g = blockIdx.x * TK_THREADS + threadIdx.x;
  if (g >= K) return;
  if (!touched[g]) {
    label[g] = -1;
    return;
  }
  const int r = tk_find(parent, g);
  label[g] = r;
  const uint32_t bit = 1u << tk_view(offs, V, g);
  const uint32_t old = atomicOr(seen + r, bit);
  if (old & bit) atomicOr(conflict + r, bit);   // a second node of that view
}

// the views a component keeps under the policy, and whether it survives the conflict rule
__device__ __forceinline__ uint32_t tk_views_left(uint32_t seen, uint32_t conf, int policy, bool* alive) {
  *alive = policy != 0 || conf == 0u;
  return policy != 0 ? seen & ~conf : seen;
}

__global__ __launch_bounds__(TK_THREADS) void tk_flag_kernel(int K, int min_views, int policy, const int32_t* __restrict__ label,
                                                             const uint32_t* __restrict__ seen, const uint32_t* __restrict__ conflict,
                                                             int32_t* __restrict__ parent, int32_t* __restrict__ bsum,
                                                             int32_t* __restrict__ cnt) {
  __shared__ int sums[TK_WAVES];
  const int g = blockIdx.x * TK_THREADS + threadIdx.x;
  const bool root = g < K && label[g] == g;
  bool alive = false;
  uint32_t conf = 0u, left = 0u;
  if (root) conf = conflict[g], left = tk_views_left(seen[g], conf, policy, &alive);
  const bool is_short = root && alive && __popc(left) < min_views;
  const int flag = root && alive && !is_short ? 1 : 0;
  int total;
  const int before = cotr_scan::block_scan<TK_WAVES>(flag, sums, &total);
  if (g < K) parent[g] = flag ? before : -1;
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
  const int nc = tk_wave_sum(root ? 1 : 0), nf = tk_wave_sum(root && conf != 0u ? 1 : 0), ns = tk_wave_sum(is_short ? 1 : 0);
  if ((threadIdx.x & 63) == 0) {
    if (nc) atomicAdd(cnt + TK_CNT_COMP, nc);
    if (nf) atomicAdd(cnt + TK_CNT_CONF, nf);
    if (ns) atomicAdd(cnt + TK_CNT_SHORT, ns);
  }
}

__global__ __launch_bounds__(TK_THREADS) void tk_scan_kernel(int blocks, int cap, int32_t* __restrict__ bsum, const int32_t* __restrict__ cnt,
                                                             int32_t* __restrict__ info) {
  __shared__ int sums[TK_WAVES];
  const int total = cotr_scan::scan_array<TK_WAVES>(
      blocks, sums, [&](int i) { return bsum[i]; }, [&](int i, int before) { bsum[i] = before; });
  if (threadIdx.x != 0) return;
  info[0] = total, info[1] = total < cap ? total : cap, info[2] = 0;
  info[3] = cnt[TK_CNT_LIVE], info[4] = cnt[TK_CNT_COMP], info[5] = cnt[TK_CNT_CONF], info[6] = cnt[TK_CNT_SHORT], info[7] = 0;
}

__global__ __launch_bounds__(TK_THREADS) void tk_fill_kernel(int cells, int32_t* __restrict__ node_out, uint8_t* __restrict__ visible_out,
                                                             double* __restrict__ points_out) {
  const int i = blockIdx.x * TK_THREADS + threadIdx.x;
  if (i >= cells) return;
  node_out[i] = -1, visible_out[i] = 0;
  if (points_out) points_out[2 * (size_t)i] = NAN, points_out[2 * (size_t)i + 1] = NAN;
}

// A written track holds at most one node of a view it keeps (two would put the view in conflict), so cell (view, track) has one
// writer.
__global__ __launch_bounds__(TK_THREADS) void tk_scatter_kernel(const int32_t* __restrict__ offsets, const double* __restrict__ keypoints,
                                                                int V, int K, int policy, int cap, const int32_t* __restrict__ label,
                                                                const int32_t* __restrict__ pos, const int32_t* __restrict__ bsum,
                                                                const uint32_t* __restrict__ seen, const uint32_t* __restrict__ conflict,
                                                                int32_t* __restrict__ track_of_node, int32_t* __restrict__ node_out,
                                                                uint8_t* __restrict__ visible_out, double* __restrict__ points_out,
                                                                int32_t* __restrict__ info) {
  __shared__ int offs[TK_MAX_VIEWS + 1];
  tk_load_offsets(offs, offsets, V);
  __syncthreads();
  const int g = blockIdx.x * TK_THREADS + threadIdx.x;
  int t = -1, views = 0;
  if (g < K) {
    const int r = label[g];
    if (r >= 0 && pos[r] >= 0) {
      const int v = tk_view(offs, V, g);
      const uint32_t conf = conflict[r];
      const int col = bsum[r / TK_THREADS] + pos[r];
      if (col < cap) {
        if (r == g) {   // the root speaks for the track, also when its own view is in conflict
          bool alive;
          views = __popc(tk_views_left(seen[r], conf, policy, &alive));
        }
        if (policy == 0 || !(conf >> v & 1u)) {
          t = col;
          const size_t cell = (size_t)v * cap + t;
          node_out[cell] = g - offs[v];
          visible_out[cell] = 1;
          if (points_out) points_out[2 * cell] = keypoints[2 * (size_t)g], points_out[2 * cell + 1] = keypoints[2 * (size_t)g + 1];
        }
      }
    }
    track_of_node[g] = t;
  }
  const int n = tk_wave_sum(t >= 0 ? 1 : 0);
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(info + 2, n);
  if (views) atomicMax(info + 7, views);
}

// ---- host side ------------------------------------------------------------------------------------------------------------
namespace {

const char* const TK_FN = "cotr_build_tracks";

const char* tk_check_shape(int K, int M) {
  if (K < 1 || K > TK_MAX_NODES) return "K must be in [1, 2^21]";
  if (M < 0 || M > TK_MAX_MATCHES) return "M must be in [0, 2^24]";
  return nullptr;
}

}  // namespace

extern "C" {

int cotr_build_tracks_work_ints(int K, int M, size_t* ints) {
  if (!ints) return arg_fail("cotr_build_tracks_work_ints", "ints is NULL");
  if (const char* msg = tk_check_shape(K, M)) return arg_fail(TK_FN, msg);
  *ints = tk_layout(nullptr, K, M).ints;
  return COTR_OK;
}

int cotr_build_tracks(const int32_t* offsets, const int32_t* matches, const uint8_t* keep, const double* keypoints, int V, int K, int M,
                      int min_views, int conflict, int cap, int32_t* track_of_node, int32_t* node_out, uint8_t* visible_out,
                      double* points_out, int32_t* info_out, int32_t* work_out, cotr_stream stream) {
  if (V < 2 || V > TK_MAX_VIEWS) return arg_fail(TK_FN, "V must be in [2, 32]");
  if (const char* msg = tk_check_shape(K, M)) return arg_fail(TK_FN, msg);
  if (min_views < 2 || min_views > V) return arg_fail(TK_FN, "min_views must be in [2, V]");
  if (conflict != 0 && conflict != 1) return arg_fail(TK_FN, "conflict must be 0 (drop) or 1 (views)");
  if (cap < 0 || cap > K / 2) return arg_fail(TK_FN, "cap must be in [0, K / 2]");
  if (!offsets || !track_of_node || !info_out || !work_out || (M > 0 && !matches) || (cap > 0 && (!node_out || !visible_out)))
    return arg_fail(TK_FN, "offsets, matches (M > 0), track_of_node, node_out and visible_out (cap > 0), info_out and work_out must not be NULL");
  if (cap > 0 && (keypoints == nullptr) != (points_out == nullptr)) return arg_fail(TK_FN, "points_out must be NULL exactly when keypoints is NULL");
  if (!aligned(keypoints, 8) || !aligned(points_out, 8) || !aligned(offsets, 4) || !aligned(matches, 4) || !aligned(track_of_node, 4) ||
      !aligned(node_out, 4) || !aligned(info_out, 4) || !aligned(work_out, 4))
    return arg_fail(TK_FN, "doubles must be 8-byte and ints 4-byte aligned");
  const TkWork l = tk_layout(work_out, K, M);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned nodes = (unsigned)((K + TK_THREADS - 1) / TK_THREADS);
  const unsigned mblocks = (unsigned)(M > 0 ? (M + TK_THREADS - 1) / TK_THREADS : 1);
  const int cells = V * cap;
  const unsigned cblocks = (unsigned)(cells > 0 ? (cells + TK_THREADS - 1) / TK_THREADS : 1);
  hipLaunchKernelGGL(tk_init_kernel, dim3(nodes), dim3(TK_THREADS), 0, s, K, l.parent, l.seen, l.conflict, l.touched, l.cnt);
  hipLaunchKernelGGL(tk_hook_kernel, dim3(mblocks), dim3(TK_THREADS), 0, s, offsets, matches, keep, V, K, M, l.parent, l.touched, l.cnt);
  hipLaunchKernelGGL(tk_label_kernel, dim3(nodes), dim3(TK_THREADS), 0, s, offsets, V, K, l.parent, (const uint8_t*)l.touched,
                     l.label, l.seen, l.conflict);
  hipLaunchKernelGGL(tk_flag_kernel, dim3(nodes), dim3(TK_THREADS), 0, s, K, min_views, conflict, (const int32_t*)l.label,
                     (const uint32_t*)l.seen, (const uint32_t*)l.conflict, l.parent, l.bsum, l.cnt);
  hipLaunchKernelGGL(tk_scan_kernel, dim3(1), dim3(TK_THREADS), 0, s, (int)nodes, cap, l.bsum, (const int32_t*)l.cnt, info_out);
  hipLaunchKernelGGL(tk_fill_kernel, dim3(cblocks), dim3(TK_THREADS), 0, s, cells, node_out, visible_out, cap > 0 ? points_out : nullptr);
  hipLaunchKernelGGL(tk_scatter_kernel, dim3(nodes), dim3(TK_THREADS), 0, s, offsets, keypoints, V, K, conflict, cap, (const int32_t*)l.label,
                     (const int32_t*)l.parent, (const int32_t*)l.bsum, (const uint32_t*)l.seen, (const uint32_t*)l.conflict, track_of_node,
                     node_out, visible_out, cap > 0 ? points_out : nullptr, info_out);
  return launched();
}

}  // extern "C"
