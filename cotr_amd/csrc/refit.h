// The frame of the Gauss-Newton refits on the inliers (homography.hip, pnp.hip, essential.hip: cotr_refine_pose): pairs of
// rf_accum_kernel<T> and the estimator's own finish kernel, which is rf_reduce + rf_step + its epilogue.  Rules in DESIGN.md 3h.
// rigid3d.hip uses the accumulate / reduce half alone, with two terms policies a round: its refit is a closed form, not a step.
// A terms policy T is a struct with
//   SUMS, STRIDE      the sums one launch makes, the row length of the per-chunk sums `parts` (>= SUMS)
//   Points, State     what the kernel reads the points from (by value), the refit's state in scratch
//   terms(st, pts, p, acc)   loads point p and adds its terms to acc[SUMS]
// The sums of a Gauss-Newton launch over PARAMS parameters: the upper triangle of J^T J row-major (rf_tri), J^T r, the squared
// error, then the policy's own counts.  The state is the model of the step: a struct derived from RfCore (a pose: from RfPose)
// with PARAMS, save(st), restore(st), apply(st, d), and whichever of RfCore's hooks it needs to differ in.
// Included by translation units compiled with -ffp-contract=off.
#pragma once
#include "ransac.h"
#include "rodrigues.h"

// index of (i, j), i <= j, in the row-major upper triangle of an N x N matrix
template <int N>
RS_HD constexpr int rf_tri(int i, int j) {
  return i * N - i * (i - 1) / 2 + (j - i);
}

// What every refit's state starts with, and the hooks of rf_step a model may replace.
struct RfCore {
  double err_prev;             // squared error at the parameters saved before the step on trial
  int done;                    // nothing more to accumulate
  int kept;                    // Gauss-Newton steps kept
  int trial;                   // the parameters are a step whose error is not known yet
  // whether the sums allow the step on trial to be kept at all (its error must have fallen besides)
  static __device__ __forceinline__ bool acceptable(const RfCore*, const double*) { return true; }
  // whether a further step may be solved for
  static __device__ __forceinline__ bool solvable(const RfCore*, int) { return true; }
  // the sums are those of parameters that stay: a kept step, or the first evaluation
  static __device__ __forceinline__ void evaluated(RfCore*, const double*) {}
  // the step on trial, if any, has been judged
  static __device__ __forceinline__ void judged(RfCore*) {}
};

// The part of a state that is a pose (pnp.hip, essential.hip): R, t, their copies before the step on trial, the rotation step.
struct RfPose : RfCore {
  double R[9], t[3];           // current pose
  double Rprev[9], tprev[3];   // the pose before the step on trial
  static __device__ __forceinline__ void save(RfPose* st) {
    for (int i = 0; i < 9; ++i) st->Rprev[i] = st->R[i];
    for (int i = 0; i < 3; ++i) st->tprev[i] = st->t[i];
  }
  static __device__ __forceinline__ void restore(RfPose* st) {
    for (int i = 0; i < 9; ++i) st->R[i] = st->Rprev[i];
    for (int i = 0; i < 3; ++i) st->t[i] = st->tprev[i];
  }
  // R <- exp([w]x) R
  static __device__ __forceinline__ void rotate(RfPose* st, const double* w) {
    double R[9];
    for (int i = 0; i < 9; ++i) R[i] = st->R[i];
    rodrigues_rotate(w, R);
    for (int i = 0; i < 9; ++i) st->R[i] = R[i];
  }
};

// per RS_CHUNK-point chunk: T::SUMS sums over the mask, every thread over its points in ascending order, every wavefront in a
// fixed butterfly, the 4 wavefronts in order -> parts[chunk][T::STRIDE]
template <class T>
__global__ __launch_bounds__(RS_COUNT_THREADS) void rf_accum_kernel(typename T::Points pts, int n, const uint8_t* __restrict__ mask,
                                                                    const typename T::State* __restrict__ st, double* __restrict__ parts) {
  constexpr int NS = T::SUMS;
  __shared__ double sh[RS_COUNT_THREADS / 64][T::STRIDE];
  if (st->done) return;   // uniform
  double acc[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) acc[k] = 0.0;
  const int base = blockIdx.x * RS_CHUNK;
#pragma unroll 1
  for (int s = 0; s < RS_COUNT_STEPS; ++s) {
    const int p = base + s * RS_COUNT_THREADS + threadIdx.x;
    if (p < n && mask[p]) T::terms(st, pts, p, acc);
  }
#pragma unroll
  for (int k = 0; k < NS; ++k) acc[k] = rs_wave_sum(acc[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < NS; ++k) sh[threadIdx.x >> 6][k] = acc[k];
  }
  __syncthreads();
  if ((int)threadIdx.x < NS) {
    double a = sh[0][threadIdx.x];
    for (int w = 1; w < RS_COUNT_THREADS / 64; ++w) a = a + sh[w][threadIdx.x];
    parts[(size_t)blockIdx.x * T::STRIDE + threadIdx.x] = a;
  }
}

// The head of a finish kernel (one workgroup): thread tid < ns adds the chunks in chunk order -> sums[tid] (LDS).  ns = 0: none.
template <int STRIDE>
__device__ __forceinline__ void rf_reduce(const double* __restrict__ parts, int chunks, int ns, double* sums) {
  const int tid = threadIdx.x;
  if (tid < ns) {
    double a = 0.0;
    for (int c = 0; c < chunks; ++c) a = a + parts[(size_t)c * STRIDE + tid];
    sums[tid] = a;
  }
  __syncthreads();
}

// One thread, on the sums at the current parameters: a step on trial is kept when its error fell (and the model accepts the
// sums), otherwise undone, which ends the refinement; unless this is the chain's last launch, the next step is solved for,
// the parameters saved and the step applied on trial; a degenerate system ends the refinement too.
template <class M>
__device__ __forceinline__ void rf_step(M* st, const double* sums, bool last, int round = 0) {
  constexpr int N = M::PARAMS, TRI = N * (N + 1) / 2;
  __shared__ double S[N * (N + 1)];
  __shared__ int P[N];
  const double err = sums[TRI + N];
  bool go_on = true;
  if (st->trial) {
    if (M::acceptable(st, sums) && err < st->err_prev) {
      st->kept = st->kept + 1;
      M::evaluated(st, sums);
    } else {   // not smaller (or NaN): undo the step
      M::restore(st);
      go_on = false;
    }
    st->trial = 0;
  } else {
    M::evaluated(st, sums);
  }
  M::judged(st);
  if (go_on && !last) {
    bool solved = false;
    double d[N];
    if (M::solvable(st, round)) {
      for (int i = 0; i < N; ++i) {
        for (int j = i; j < N; ++j) S[i * (N + 1) + j] = S[j * (N + 1) + i] = sums[rf_tri<N>(i, j)];
        S[i * (N + 1) + N] = -sums[TRI + i];
      }
      solved = rs_solve<N, 1>(S, P, d);
    }
    if (solved) {
      M::save(st);
      st->err_prev = err;
      M::apply(st, d);
      st->trial = 1;
    } else {
      go_on = false;
    }
  }
  if (!go_on || last) st->done = 1;
}

// ---- host side ------------------------------------------------------------------------------------------------------------
namespace cotr_detail {

// after `before` bytes of the caller's scratch: the state, then the per-chunk sums [chunks][stride]
struct RfPlan {
  size_t state, parts, bytes;
  int chunks;
};

inline RfPlan rf_plan(size_t before, size_t state_bytes, int n, int stride) {
  RfPlan l;
  l.chunks = (n + RS_CHUNK - 1) / RS_CHUNK;
  l.state = before;
  l.parts = l.state + align_up(state_bytes);
  l.bytes = l.parts + align_up((size_t)l.chunks * stride * sizeof(double));
  return l;
}

// rf_accum_kernel<T>, then one workgroup of the estimator's finish kernel: finish(chunks, parts, st, args...)
template <class T, class Finish, class... Args>
inline void rf_enqueue_pair(hipStream_t s, const RfPlan& l, void* scratch, const typename T::Points& pts, int n, const uint8_t* mask,
                            Finish finish, Args... args) {
  auto* st = reinterpret_cast<typename T::State*>(static_cast<char*>(scratch) + l.state);
  double* parts = reinterpret_cast<double*>(static_cast<char*>(scratch) + l.parts);
  hipLaunchKernelGGL(rf_accum_kernel<T>, dim3((unsigned)l.chunks), dim3(RS_COUNT_THREADS), 0, s, pts, n, mask, st, parts);
  hipLaunchKernelGGL(finish, dim3(1), dim3(64), 0, s, l.chunks, (const double*)parts, st, args...);
}

}  // namespace cotr_detail
