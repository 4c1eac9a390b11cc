// Integer prefix sums for the kernels that give every output its position: over the 64 lanes of a wavefront,
// over a workgroup, and over an array walked by one workgroup.  T is int, long long, or int2 for two counts carried together.
// Sums of integers: every order of additions gives the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace cotr_scan {

template <class T>
__device__ __forceinline__ T lanes_up(T v, int d) {
  return __shfl_up(v, d, 64);
}
__device__ __forceinline__ int2 lanes_up(int2 v, int d) { return make_int2(__shfl_up(v.x, d, 64), __shfl_up(v.y, d, 64)); }

// 1. the inclusive scan of v over the lanes of a wavefront; every lane calls it
template <class T>
__device__ __forceinline__ T wave_scan(T v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T t = lanes_up(v, d);
    if (lane >= d) v = v + t;
  }
  return v;
}

// 2. Over a workgroup: lane 63 of every wavefront leaves its wave_scan value in sums[slot], and after a barrier the sums below a
// slot are what came before that wavefront; slot = SLOTS gives the total.  A slot is the wavefront's index, or round * waves +
// index when a thread scans several values behind one barrier (ms_count_kernel).
template <class T>
__device__ __forceinline__ void wave_sum_put(T incl, T* sums, int slot) {
  if ((threadIdx.x & 63) == 63) sums[slot] = incl;
}

template <int SLOTS, class T>
__device__ __forceinline__ T wave_sums_below(const T* sums, int slot) {
  T s = T();
#pragma unroll
  for (int q = 0; q < SLOTS; ++q)
    if (q < slot) s = s + sums[q];
  return s;
}

// The exclusive offset of v among the values of a workgroup of WAVES wavefronts, and their sum in *total; sums holds WAVES
// values in LDS.  Contains ONE __syncthreads, between the store of the wave sums and their reads.  The caller owes a second one
// before sums is written again (the next call included), and none when the kernel ends first.
template <int WAVES, class T>
__device__ __forceinline__ T block_scan(T v, T* sums, T* total) {
  const int wave = threadIdx.x >> 6;
  const T incl = wave_scan(v);
  wave_sum_put(incl, sums, wave);
  __syncthreads();
  *total = wave_sums_below<WAVES>(sums, WAVES);
  return wave_sums_below<WAVES>(sums, wave) + incl - v;
}

// 3. One workgroup of WAVES wavefronts walks load(0) .. load(n - 1) in chunks of its width with a running carry: store(i, the sum
// of the values before i) for every i, and the sum of all of them returned to every thread.  load(i) and store(i, .) are called by
// one thread each, with i < n; they may alias (a thread loads its value before it stores its offset).
template <int WAVES, class T, class Load, class Store>
__device__ __forceinline__ T scan_array(int n, T* sums, Load load, Store store) {
  T carry = T();
  for (int base = 0; base < n; base += WAVES * 64) {
    const int i = base + threadIdx.x;
    T total;
    const T before = block_scan<WAVES>(i < n ? load(i) : T(), sums, &total);
    if (i < n) store(i, carry + before);
    carry = carry + total;
    __syncthreads();   // sums is written again
  }
  return carry;
}

}  // namespace cotr_scan
