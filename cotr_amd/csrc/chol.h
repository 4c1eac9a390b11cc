// The dense solve of the joint Gauss-Newton steps (bundle.hip: ba_solve_kernel, icp_multi.hip: im_solve_kernel), stated once: an
// m x m system as its packed lower triangle in LDS with the right-hand side carried as row m, Cholesky by columns over one workgroup of
// THREADS = 256 that calls uniformly, and the back substitution.  Every entry is updated by one thread, column after column: the same
// system gives the same bits.  Include only from files compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// the packed lower triangle with one more row: row i, column j <= i
__device__ __forceinline__ int ch_tri(int i, int j) { return i * (i + 1) / 2 + j; }

// L <- its Cholesky factor, row m <- the forward solve L y = b.  admit(col, pivot), called uniformly with every column's pivot before
// its square root is taken, says whether to go on; false at the first pivot it refuses (L is then half done).  Ends with a barrier.
// (global_pose.hip solves one factor for many right-hand sides: ch_forward below puts a fresh one through the same forward solve.)
template <int THREADS, class Admit>
__device__ __forceinline__ bool ch_factor(double* L, int m, Admit admit) {
  static_assert(THREADS == 256, "the trailing update runs on a 16 x 16 grid of threads");
  const int tid = threadIdx.x;
  bool ok = true;
  for (int col = 0; col < m; ++col) {
    __syncthreads();
    const double pivot = L[ch_tri(col, col)];
    if (!admit(col, pivot)) {   // uniform
      ok = false;
      break;
    }
    const double d = sqrt(pivot);
    __syncthreads();
    for (int i = col + tid; i <= m; i += THREADS) L[ch_tri(i, col)] = i == col ? d : L[ch_tri(i, col)] / d;
    __syncthreads();
    // the trailing update on a 16 x 16 grid of threads: rows col+1 .. m (row m: the right-hand side), columns col+1 .. min(row, m-1)
    for (int i = col + 1 + (tid >> 4); i <= m; i += 16) {
      const double lik = L[ch_tri(i, col)];
      const int end = i < m ? i : m - 1;
      for (int j = col + 1 + (tid & 15); j <= end; j += 16) L[ch_tri(i, j)] -= lik * L[ch_tri(j, col)];
    }
  }
  __syncthreads();
  return ok;
}

// A fresh right-hand side b in row m of a factor ch_factor returned true for: row m <- the forward solve L y = b, by the operations
// ch_factor applies to that row (the division by the column's diagonal entry, then one update per entry by one thread), so the same b
// gives the bits ch_factor would have left.  Begins and ends with a barrier.
template <int THREADS>
__device__ __forceinline__ void ch_forward(double* L, int m) {
  const int tid = threadIdx.x;
  for (int col = 0; col < m; ++col) {
    __syncthreads();
    const double y = L[ch_tri(m, col)] / L[ch_tri(col, col)];
    __syncthreads();
    if (tid == 0) L[ch_tri(m, col)] = y;
    for (int j = col + 1 + tid; j < m; j += THREADS) L[ch_tri(m, j)] -= y * L[ch_tri(j, col)];
  }
  __syncthreads();
}

// L^T x = y, y in row m -> xs[0 .. m-1] (complete for every thread on return), after ch_factor returned true.  One barrier a column
// suffices: column col reads L[m][col], L[col][col] and writes only L[m][i], i < col, so every update of L[m][col] precedes the barrier that ends an earlier column.
template <int THREADS>
__device__ __forceinline__ void ch_back(double* L, int m, double* xs) {
  const int tid = threadIdx.x;
  for (int col = m - 1; col >= 0; --col) {
    const double x = L[ch_tri(m, col)] / L[ch_tri(col, col)];
    if (tid == 0) xs[col] = x;
    for (int i = tid; i < col; i += THREADS) L[ch_tri(m, i)] -= L[ch_tri(col, i)] * x;
    __syncthreads();
  }
}
