// The pieces the RANSAC estimators share (guided.hip: fundamental matrix, homography.hip: homography, essential.hip:
// essential matrix): the counter-based sampler, OpenCV's iteration update, the kernel that replays the sequential selection
// loop on the counts, and the cyclic Jacobi iteration of the symmetric eigenproblems.  Rules in DESIGN.md 3h.  Included by translation units compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#define RS_MAX_DRAWS 64
#define RS_SOLVE_THREADS 64
#define RS_COUNT_THREADS 256
#define RS_COUNT_STEPS 8       // points per thread per workgroup: chunks of 2048 points
#define RS_CHUNK (RS_COUNT_THREADS * RS_COUNT_STEPS)
#define RS_SELECT_THREADS 1024
#define RS_MAX_ITERS (1 << 16)
#define RS_MAX_POINTS (1 << 24)
#define RS_RANK_TOL 1e-12      // a pivot below this times the first one: the sample is degenerate
#define RS_JACOBI_SWEEPS 30

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ double f32r(double v) { return (double)(float)v; }

// Sample of iteration it: draw d is splitmix64(splitmix64(seed) ^ (it << 6 | d)), index (z >> 32) % n; duplicates are
// rejected; the first MODEL distinct indices of at most RS_MAX_DRAWS draws go to s[k * stride].  Returns how many it got.
template <int MODEL>
__device__ __forceinline__ int rs_sample(uint64_t seed, int it, int n, int* s, int stride) {
  const uint64_t sk = splitmix64(seed);
  int got = 0;
  for (int d = 0; d < RS_MAX_DRAWS && got < MODEL; ++d) {
    const uint64_t z = splitmix64(sk ^ (((uint64_t)it << 6) | (uint64_t)d));
    const int c = (int)((z >> 32) % (uint64_t)n);
    bool dup = false;
    for (int k = 0; k < got; ++k) dup = dup || s[k * stride] == c;
    if (!dup) {
      s[got * stride] = c;
      ++got;
    }
  }
  return got;
}

// OpenCV's RANSACUpdateNumIters
__device__ inline int ransac_update(double p, double ep, int m, int N) {
  const double num = log(fmax(1.0 - p, DBL_MIN));
  const double denom = 1.0 - pow(1.0 - ep, (double)m);
  if (denom < DBL_MIN) return 0;
  const double lden = log(denom);
  return (lden >= 0.0 || -num >= (double)N * (-lden)) ? N : (int)rint(num / lden);
}

// Cyclic Jacobi on the symmetric N x N a: rotations (p, q) in row-major order until the off-diagonal norm falls below
// DBL_EPSILON times the Frobenius norm, at most RS_JACOBI_SWEEPS sweeps.  a ends (nearly) diagonal with the eigenvalues, the
// columns of v are the eigenvectors.  One thread.
template <int N>
__device__ void rs_jacobi(double (*a)[N], double (*v)[N]) {
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) v[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < RS_JACOBI_SWEEPS; ++sweep) {
    double off = 0.0, all = 0.0;
    for (int i = 0; i < N; ++i)
      for (int j = 0; j < N; ++j) {
        const double t = a[i][j] * a[i][j];
        all += t;
        if (i != j) off += t;
      }
    if (!(sqrt(off) >= DBL_EPSILON * sqrt(all))) break;   // converged (or NaN)
    for (int p = 0; p < N - 1; ++p)
      for (int q = p + 1; q < N; ++q) {
        const double apq = a[p][q];
        if (apq == 0.0) continue;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
        const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < N; ++k) {   // columns p and q
          const double akp = a[k][p], akq = a[k][q];
          a[k][p] = c * akp - s * akq;
          a[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < N; ++k) {   // rows p and q
          const double apk = a[p][k], aqk = a[q][k];
          a[p][k] = c * apk - s * aqk;
          a[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < N; ++k) {
          const double vkp = v[k][p], vkq = v[k][q];
          v[k][p] = c * vkp - s * vkq;
          v[k][q] = s * vkp + c * vkq;
        }
      }
  }
}

// The sequential loop, replayed: the next slot that beats max(best, MODEL - 1) within the iterations still to run is found
// by a parallel minimum over the slots after the last one taken.  SLOTS candidates per iteration (slot = SLOTS * it + k).
// info = {found, best, iterations run, chosen slot}.
template <int MODEL, int SLOTS>
__global__ __launch_bounds__(RS_SELECT_THREADS) void rs_select_kernel(const int* __restrict__ count, int max_iters, int n, double confidence,
                                                                      int32_t* __restrict__ info, int32_t* __restrict__ hyp_count) {
  __shared__ int st[4];   // next slot to look at (-1: done), best, niters, chosen slot
  __shared__ int red[RS_SELECT_THREADS / 64];
  const int tid = threadIdx.x;
  const int nslots = SLOTS * max_iters;
  if (hyp_count)
    for (int s = tid; s < nslots; s += RS_SELECT_THREADS) hyp_count[s] = count[s];
  if (tid == 0) st[0] = 0, st[1] = 0, st[2] = max_iters, st[3] = -1;
  __syncthreads();
  for (;;) {
    const int pos = st[0], best = st[1], niters = st[2], chosen = st[3];
    if (pos < 0) break;   // uniform
    const int thr = max(best, MODEL - 1);
    // slots of the iterations it < niters, and the rest of the iteration of the last slot taken
    const int limit = SLOTS * max(niters, chosen >= 0 ? chosen / SLOTS + 1 : 0);
    int local = INT_MAX;
    for (int s = pos + tid; s < limit; s += RS_SELECT_THREADS)
      if (count[s] > thr) {
        local = s;
        break;
      }
    for (int off = 32; off > 0; off >>= 1) local = min(local, __shfl_xor(local, off));
    if ((tid & 63) == 0) red[tid >> 6] = local;
    __syncthreads();
    if (tid == 0) {
      int m = INT_MAX;
      for (int w = 0; w < RS_SELECT_THREADS / 64; ++w) m = min(m, red[w]);
      if (m == INT_MAX) {
        st[0] = -1;
      } else {
        const int nb = count[m];
        st[0] = m + 1;
        st[1] = nb;
        st[2] = ransac_update(confidence, (double)(n - nb) / (double)n, MODEL, niters);
        st[3] = m;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int chosen = st[3];
    info[0] = chosen >= 0 ? 1 : 0;
    info[1] = st[1];
    info[2] = chosen >= 0 ? max(st[2], chosen / SLOTS + 1) : max_iters;
    info[3] = chosen;
  }
}
