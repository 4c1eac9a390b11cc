// ln_reduce_kernel (pointwise.hip) for the two slab counts of the forward path, 8 (attention heads) and 16 (fused-FFN chunks), with
// its dependent memory round trips taken out: the 24 ln_reduce launches of a one-pair forward are bound by the latency chain inside each
// launch (argument loads -> bias / residual -> slabs [-> slabs again] -> 12 trips through the LDS crossbar for the two wave sums), not by
// their bytes.  Here
//   * the arguments are ONE by-value struct: one batch of scalar loads, issued before the row guard is tested;
//   * every global load of the launch (bias, residual, all NP slabs, w, b [, post_w, post_b]) is issued before the first wait - the slab
//     count is a template parameter, so there is no slab loop; a null residual loads the bias row again and discards it (a select, no
//     branch around the load);
//   * the wave sums exchange lanes with v_permlane32_swap / v_permlane16_swap and DPP row operations instead of ds_bpermute_b32.
// The arithmetic is ln_reduce_kernel's, operation for operation (sum order bias + residual, slabs 0..NP-1; mean, then the variance of the
// centred values; 1.f / sqrtf(var + 1e-5f); d * rstd * w + b), and the wave sums pair the lanes as its xor butterfly does (32, 16, 8, 4,
// 2, 1): the results are the same bits (tests/test_ln_reduce1_gpu.py).  ln_reduce_kernel stays the reference and serves every other np.
#include "common.h"

struct LnReduce1Args {
  const float* parts;
  const float* bias;
  const float* residual;   // may be nullptr
  float* y;                // (in front of the pointers only some instantiations read: every instantiation's arguments are one contiguous run)
  const float* w;
  const float* b;
  const float* post_w;     // read only by the POST instantiations
  const float* post_b;
  int rows;
};

// lane i <-> lane i ^ 32 / i ^ 16 without the LDS crossbar: both operands hold v; the swap exchanges lanes 32-63 (odd rows of 16) of the
// first register with lanes 0-31 (even rows) of the second, so every lane ends with its own value in one and its partner's in the other.
// Inline asm, as in att_rows.hip: given the same value for both operands the builtin keeps only its first result.  s_nop 1: the two wait
// states between a VALU write of an operand and the swap that reads it.
__device__ __forceinline__ float ln1_xor32_sum(float v) {
  float a = v, b = v;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
  return a + b;
}
__device__ __forceinline__ float ln1_xor16_sum(float v) {
  float a = v, b = v;
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
  return a + b;
}
template <int CTRL>
__device__ __forceinline__ float ln1_dpp_sum(float v) {
  return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
// wave_sum (pointwise.hip) with the same pairing: each step adds the value of lane i ^ off to lane i's (fp addition is commutative, so
// both partners get the same bits).  row_ror:8 is lane i ^ 8 of a row of 16; after that step a value depends on i % 8 only, so row_ror:4
// (lane (i + 4) % 16) delivers the value of lane i ^ 4; the quad permutations are i ^ 2 and i ^ 1.
__device__ __forceinline__ float ln1_wave_sum(float v) {
  v = ln1_xor32_sum(v);
  v = ln1_xor16_sum(v);
  v = ln1_dpp_sum<0x128>(v);   // row_ror:8
  v = ln1_dpp_sum<0x124>(v);   // row_ror:4
  v = ln1_dpp_sum<0x4E>(v);    // quad_perm [2,3,0,1]
  v = ln1_dpp_sum<0xB1>(v);    // quad_perm [1,0,3,2]
  return v;
}

// The row guard is a clamp and a predicated store, not an early return: with a branch on `rows` in front, the compiler fetches `rows`
// alone, waits, and only then requests the other arguments.  (The wavefronts past the last row of a ragged last workgroup recompute that
// row and store nothing.)  amdgpu_waves_per_eu(1, 4): up to 128 VGPRs, so the 16-slab form keeps all its loads in flight at once instead
// of recycling registers between waits; sched_barrier: no load sinks below the first add, so the first wait comes after the last load.
template <int NP, bool POST>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 4))) void ln_reduce1_kernel(const LnReduce1Args a) {
  const int lane = threadIdx.x & 63;
  const int row_raw = blockIdx.x * 4 + (threadIdx.x >> 6);
  const bool live = row_raw < a.rows;
  const int row = live ? row_raw : a.rows - 1;
  const size_t roff = (size_t)row * 256 + lane * 4;
  const bool has_res = a.residual != nullptr;
  f32x4 v = *reinterpret_cast<const f32x4*>(a.bias + lane * 4);
  f32x4 rr = *reinterpret_cast<const f32x4*>(has_res ? a.residual + roff : a.bias + lane * 4);
  const float* prow = a.parts + roff;
  const size_t pstride = (size_t)a.rows * 256;
  f32x4 t[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) t[k] = *reinterpret_cast<const f32x4*>(prow + (size_t)k * pstride);
  const f32x4 ww = *reinterpret_cast<const f32x4*>(a.w + lane * 4);
  const f32x4 bb = *reinterpret_cast<const f32x4*>(a.b + lane * 4);
  f32x4 w2 = {0.f, 0.f, 0.f, 0.f}, b2 = {0.f, 0.f, 0.f, 0.f};
  if (POST) {
    w2 = *reinterpret_cast<const f32x4*>(a.post_w + lane * 4);
    b2 = *reinterpret_cast<const f32x4*>(a.post_b + lane * 4);
  }
  __builtin_amdgcn_sched_barrier(0);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  v += has_res ? rr : zero;
#pragma unroll
  for (int k = 0; k < NP; ++k) v += t[k];
  const float mean = ln1_wave_sum(v[0] + v[1] + v[2] + v[3]) * (1.f / 256.f);
  const f32x4 d = {v[0] - mean, v[1] - mean, v[2] - mean, v[3] - mean};
  const float var = ln1_wave_sum(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3]) * (1.f / 256.f);
  const float rstd = 1.f / sqrtf(var + 1e-5f);
  f32x4 out;
#pragma unroll
  for (int i = 0; i < 4; ++i) out[i] = d[i] * rstd * ww[i] + bb[i];
  if (POST) {   // decoder.norm after the last layer's norm3 (transformer.py:110-111)
    const float m2 = ln1_wave_sum(out[0] + out[1] + out[2] + out[3]) * (1.f / 256.f);
    const f32x4 d2 = {out[0] - m2, out[1] - m2, out[2] - m2, out[3] - m2};
    const float v2 = ln1_wave_sum(d2[0] * d2[0] + d2[1] * d2[1] + d2[2] * d2[2] + d2[3] * d2[3]) * (1.f / 256.f);
    const float r2 = 1.f / sqrtf(v2 + 1e-5f);
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = d2[i] * r2 * w2[i] + b2[i];
  }
  if (live) *reinterpret_cast<f32x4*>(a.y + roff) = out;
}

bool ln_reduce1_applies(int np) { return np == 8 || np == 16; }

// launch_ln_reduce_post's signature; np must be 8 or 16 (launch_ln_reduce_post forwards exactly those)
int launch_ln_reduce1(const float* parts, int np, const float* bias, const float* residual, const float* w, const float* b,
                      const float* post_w, const float* post_b, float* y, int rows, hipStream_t s) {
  if (!ln_reduce1_applies(np)) return -1;
  if (rows <= 0) return 0;
  const LnReduce1Args a = {parts, bias, residual, y, w, b, post_w, post_b, rows};
  const dim3 grid((rows + 3) / 4), block(256);
  const bool post = post_w != nullptr;
  if (np == 8) {
    if (post) hipLaunchKernelGGL((ln_reduce1_kernel<8, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((ln_reduce1_kernel<8, false>), grid, block, 0, s, a);
  } else {
    if (post) hipLaunchKernelGGL((ln_reduce1_kernel<16, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((ln_reduce1_kernel<16, false>), grid, block, 0, s, a);
  }
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
