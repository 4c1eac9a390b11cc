// The few-rows fused feed-forward launch of ffn.hip with its two phases on DIFFERENT wavefronts of the workgroup, overlapped across
// sub-chunks.  Same decomposition (grid (rows/32) x NCH, 512 threads, 32 rows x 1024/NCH hidden units per workgroup, NCH partial slabs for
// ln_reduce, write-through stores, the two workgroup orders), same floating-point operations in the same order per element - the bits of
// ffn_fused_kernel (tests/test_ffn_fused_loads_gpu.py, tests/test_ffn_pipeline_gpu.py) - only the inside of the workgroup differs:
// ffn_fused_kernel alternates  barrier | phase 1 on all 8 wavefronts | barrier | phase 2 on all 8 wavefronts,  so the matrix pipes idle under
// every fragment ds_read, the b1 load, the ReLU and H write and the wait for the slower of the two wavefronts of a SIMD (phase stamps:
// 5.4 - 6.0 us per 64 hidden units for 3.8 us of MFMA, profiles/ffn_pipeline_phases.txt).  Here a sub-chunk is 32 hidden units, NS = 1024/NCH/32
// steps, and each SIMD holds one wavefront of either role:
//   wavefronts 0-3  phase 1: H[32 x 32] = relu(X . W1_sub^T + b1) as 2 x 2 tiles of 16 x 16 (v_mfma_f32_16x16x4_f32), one tile per wavefront
//                   over the whole K = 256 with the even / odd accumulator pair of ffn_fused_kernel (64 MFMAs per step) -> Hs[step & 1];
//                   they also issue the LDS-DMA of X and of the W1 stages (three stages, two in flight)
//   wavefronts 4-7  phase 2: wavefront q owns output column blocks 2q, 2q+1 (two independent f32x16 accumulators), per step and block
//                   j = 0..3, e = 0..3 on v_mfma_f32_32x32x2_f32 from Hs and the W2 fragment in registers (32 MFMAs per step = the 2048
//                   pipe cycles of a phase-1 step); W2 goes global -> registers in ffn_fused_kernel's layout, a step's fragments two barriers ahead
// One s_barrier per step i = 0..NS in BOTH roles (NS + 1 each, whatever M): behind barrier i the phase-1 wavefronts request W1 stage i + 2
// (into the stage sub-chunk i - 1 released) and compute sub-chunk i, the phase-2 wavefronts consume Hs of sub-chunk i - 1.  Two 32-unit
// steps walk exactly j = 0..7 of one 64-unit sub-chunk of ffn_fused_kernel: ascending sub-chunk, j, e for every output element.
#include "common.h"

#define FP_D 256
#define FP_H 1024
#define FP_LD 260    // padded LDS row of 256 floats
#define FP_HLD 36    // padded LDS row of the 32-wide hidden sub-chunk

struct FfnPipeParams {
  const float* X;    // [M][256]
  const float* W1;   // [1024][256]
  const float* b1;   // [1024]
  const float* W2;   // [256][1024]
  float* P;          // [nch][M][256] partial outputs
  const float* zeros;
  int M, chunk_major;
  int wt_partials;   // partial outputs with write-through stores
  unsigned long long* dbg;  // nullptr, or [workgroups][8] phase timestamps (100 MHz wall clock), cotr_debug_ffn_times
};

template <int N>
__device__ __forceinline__ void fp_wait_vmcnt() {
  static_assert(N >= 0 && N <= 63, "vmcnt is a 6-bit counter");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// s_barrier alone (__syncthreads() is a fence too and drains the wavefront's whole memory queue: the W1 stage and the W2 fragments in
// flight).  Every wavefront retires its own LDS accesses first: the H writes must be visible, the fragment reads of a stage / an Hs
// buffer done before the other role overwrites it.
__device__ __forceinline__ void fp_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

template <int NS>
__global__ __launch_bounds__(512) void ffn_fused_pipe_kernel(const FfnPipeParams p) {
  constexpr int NCH = FP_H / 32 / NS;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Xs = smem;                       // [32][260]
  float* W1s = Xs + 32 * FP_LD;           // [3][32][260]
  float* Hs = W1s + 3 * 32 * FP_LD;       // [2][32][36]

  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int l31 = lane & 31, hh = lane >> 5;
#define FP_STAMP(slot, thread)                                                                        \
  do {                                                                                                \
    if (p.dbg != nullptr && t == (thread)) p.dbg[(size_t)blockIdx.x * 8 + (slot)] = wall_clock64();   \
  } while (0)
  FP_STAMP(0, 0);
  // chunk_major: see ffn_fused_kernel
  const int tiles = gridDim.x / NCH;
  const int chunk = p.chunk_major ? blockIdx.x % NCH : blockIdx.x / tiles;
  const int m0 = (p.chunk_major ? blockIdx.x / NCH : blockIdx.x % tiles) * 32;
  const int h0 = chunk * (FP_H / NCH);

  if (wave < 4) {
    // ---- phase-1 role ------------------------------------------------------------------------------
    const int l15 = lane & 15, q4 = lane >> 4;
    const int rb = wave & 1, cb = wave >> 1;
    // b1 of every step first: the oldest entries of this wavefront's in-order memory queue, landed with the counted wait in front of
    // barrier 0.  (asm: as plain loads hipcc waits for them with vmcnt(0) in front of the first H write - behind the two W1 stages in
    // flight - since it cannot count across the DMA instructions.)
    float b1v[NS];
    const float* b1g = p.b1 + h0 + cb * 16 + l15;
#pragma unroll
    for (int s = 0; s < NS; ++s) asm volatile("global_load_dword %0, %1, off" : "=v"(b1v[s]) : "v"(b1g + s * 32) : "memory");
    // X tile and W1 stages: one DMA row per wave instruction, 8 rows of each per wavefront
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = wave + 4 * i;
      const float* src = (m0 + row < p.M) ? p.X + (size_t)(m0 + row) * FP_D + lane * 4 : p.zeros;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                       (__attribute__((address_space(3))) void*)(Xs + row * FP_LD), 16, 0, 0);
    }
    auto dma_w1 = [&](int step) {
      float* stage = W1s + (step % 3) * (32 * FP_LD);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int row = wave + 4 * i;
        const float* src = p.W1 + (size_t)(h0 + step * 32 + row) * FP_D + lane * 4;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(stage + row * FP_LD), 16, 0, 0);
      }
    };
    dma_w1(0);
    dma_w1(1);   // NS >= 2
    FP_STAMP(1, 0);

    const float* xr = &Xs[(rb * 16 + l15) * FP_LD + q4 * 4];
    f32x4 xa[16];
#pragma unroll
    for (int i = 0; i <= NS; ++i) {
      // this wavefront's DMA of the stage step i reads (and X) has landed; stage i + 1 (8 instructions) stays in flight
      if (i + 1 < NS) fp_wait_vmcnt<8>();
      else fp_wait_vmcnt<0>();
      fp_barrier();
      if (i == 0) FP_STAMP(2, 0);
      else if (i == 1) FP_STAMP(3, 0);
      else if (i == 2) FP_STAMP(5, 0);
      if (i == NS) break;
      if (i + 2 < NS) dma_w1(i + 2);   // into the stage of sub-chunk i - 1: every phase-1 wavefront retired its reads before this barrier
      if (i == 0) {
        // the X fragments of this wavefront's 16 rows are those of every step: read once
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) xa[kk] = *reinterpret_cast<const f32x4*>(xr + kk * 16);
#pragma unroll
        for (int s = 0; s < NS; ++s) asm volatile("" : "+v"(b1v[s]));   // no use of b1 above the wait that covers its load
      }
      // the arithmetic of ffn_fused_kernel's phase 1, tile (rb, cb) of this step's 2 x 2.  The MFMA run starts on the first four W1
      // fragments, the other twelve are requested behind its first two MFMAs and land under the next fourteen: behind a DMA instruction
      // every wait hipcc inserts is a full one (lgkmcnt(0)), so what is requested in front of the run is waited for in front of it
      // (all sixteen in front: 12.30 -> 12.25 us per block at 512 rows, 17.42 -> 17.35 at 1000)
      f32x4 ae = {0.f, 0.f, 0.f, 0.f}, ao = {0.f, 0.f, 0.f, 0.f};
      const float* wr = &W1s[(i % 3) * (32 * FP_LD) + (cb * 16 + l15) * FP_LD + q4 * 4];
      f32x4 wb[16];
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) wb[kk] = *reinterpret_cast<const f32x4*>(wr + kk * 16);
      __builtin_amdgcn_sched_barrier(0);
      ae = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[0][0], wb[0][0], ae, 0, 0, 0);
      ao = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[1][0], wb[1][0], ao, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int kk = 4; kk < 16; ++kk) wb[kk] = *reinterpret_cast<const f32x4*>(wr + kk * 16);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int kk = 0; kk < 16; kk += 2) {
#pragma unroll
        for (int e = (kk == 0 ? 1 : 0); e < 4; ++e) {
          ae = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[kk][e], wb[kk][e], ae, 0, 0, 0);
          ao = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[kk + 1][e], wb[kk + 1][e], ao, 0, 0, 0);
        }
      }
      // D of 16x16x4: column = lane & 15 (hidden unit), row = (lane >> 4) * 4 + reg
      float* hw = Hs + (i & 1) * (32 * FP_HLD);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = ae[r] + ao[r] + b1v[i];
        v = (v < 0.f) ? 0.f : v;
        hw[(rb * 16 + q4 * 4 + r) * FP_HLD + cb * 16 + l15] = v;
      }
    }
    return;
  }

  // ---- phase-2 role --------------------------------------------------------------------------------
  const int q = wave - 4;
  // W2 fragments of step s, block b: lane (n = l31, half hh) holds W2[32 * (2q + b) + l31][h0 + s*32 + j*8 + hh*4 .. +3], j = 0..3
  f32x4 w2f[NS][2][4];
  const float* w2g = p.W2 + (size_t)(64 * q + l31) * FP_H + h0 + hh * 4;
  auto load_w2 = [&](int s) {
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int j = 0; j < 4; ++j) w2f[s][b][j] = *reinterpret_cast<const f32x4*>(w2g + (size_t)b * 32 * FP_H + s * 32 + j * 8);
  };
  // Requested in the order of need, step i + 1 behind barrier i (two barriers ahead of its use): a CU's intake is what the start of
  // the launch waits for, and all four steps of W2 (128 KB per workgroup at 8 chunks) requested up front stood in front of X and the
  // first W1 stage - X + W1 usable 2.1 us later, 18.8 against 17.4 us per block at 1000 rows.
  load_w2(0);
  __builtin_amdgcn_sched_barrier(0);     // requested here, not at its first use

  f32x16 acc[2];
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[0][r] = acc[1][r] = 0.f;

#pragma unroll
  for (int i = 0; i <= NS; ++i) {
    fp_barrier();
    if (i + 1 < NS) {
      load_w2(i + 1);                    // into the registers the MFMAs of step i - 2 have read
      __builtin_amdgcn_sched_barrier(0);
    }
    if (i == 0) continue;
    const float* hr = Hs + ((i - 1) & 1) * (32 * FP_HLD) + l31 * FP_HLD + hh * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 af = *reinterpret_cast<const f32x4*>(hr + j * 8);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[e], w2f[i - 1][0][j][e], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[e], w2f[i - 1][1][j][e], acc[1], 0, 0, 0);
      }
    }
    if (i == 1) FP_STAMP(4, 256);
  }
  FP_STAMP(6, 256);

  // partial output blocks of this wavefront: rows m0 + (r&3) + 8*(r>>2) + 4*hh, columns 32 * (2q + b) + l31, through a wave-private LDS
  // tile so that the rows leave as float4 (see ffn_fused_kernel).  The W1 stages are free: behind barrier NS no DMA is in flight and
  // every phase-1 wavefront is past its last read.
  float* out = p.P + (size_t)chunk * p.M * FP_D;
  const int sr = lane >> 3, sc = (lane & 7) * 4;
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    float* stage = W1s + (2 * q + b) * (32 * 36);
#pragma unroll
    for (int r = 0; r < 16; ++r) stage[((r & 3) + 8 * (r >> 2) + 4 * hh) * 36 + l31] = acc[b][r];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int row = it * 8 + sr;
      const f32x4 val = *reinterpret_cast<const f32x4*>(&stage[row * 36 + sc]);
      if (m0 + row < p.M) store_f32x4(out + (size_t)(m0 + row) * FP_D + 32 * (2 * q + b) + sc, val, p.wt_partials != 0);
    }
  }
  FP_STAMP(7, 256);
}

static const size_t kFfnPipeSmem = (size_t)(32 * FP_LD + 3 * 32 * FP_LD + 2 * 32 * FP_HLD) * sizeof(float);

static thread_local unsigned long long* g_ffn_pipe_dbg = nullptr;   // set_ffn_pipe_debug_times: phase stamps of the next launches
void set_ffn_pipe_debug_times(unsigned long long* p) { g_ffn_pipe_dbg = p; }

// which chunk counts run the pipelined form (the others: ffn_fused_kernel)
bool ffn_pipe_applies(int nch) { return nch == 2 || nch == 4 || nch == 8 || nch == 16; }

template <int NS>
static int launch_ffn_pipe_ns(const FfnPipeParams& p, int grid, hipStream_t s) {
  static PerDeviceFlag attr_set;
  if (!attr_set.get()) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(ffn_fused_pipe_kernel<NS>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)kFfnPipeSmem) != hipSuccess)
      return -2;
    attr_set.set();
  }
  hipLaunchKernelGGL(ffn_fused_pipe_kernel<NS>, dim3(grid), dim3(512), kFfnPipeSmem, s, p);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// The few-rows fused FFN launch, in the form that serves this chunk count: the ONE place that chooses between ffn_fused_pipe_kernel and
// ffn_fused_kernel (ffn_block and cotr_op_ffn_block both come through here).
int launch_ffn_few_rows(const float* X, const float* W1, const float* b1, const float* W2, float* P, int M, int nch, hipStream_t s) {
  if (!ffn_pipe_applies(nch)) return launch_ffn_fused(X, W1, b1, W2, P, M, nch, s);
  if (M <= 0) return 0;
  FfnPipeParams p;
  p.X = X; p.W1 = W1; p.b1 = b1; p.W2 = W2; p.P = P; p.zeros = gemm_zero_buffer(); p.M = M;
  p.chunk_major = (knob(KN_XCD_MAPPING) >> 2) & 1;
  p.wt_partials = ((knob(KN_XCD_MAPPING) >> 4) & 1) == 0;
  p.dbg = g_ffn_pipe_dbg;
  if (p.zeros == nullptr) return -2;
  const int grid = ((M + 31) / 32) * nch;
  switch (nch) {
    case 16: return launch_ffn_pipe_ns<2>(p, grid, s);
    case 8: return launch_ffn_pipe_ns<4>(p, grid, s);
    case 4: return launch_ffn_pipe_ns<8>(p, grid, s);
    default: return launch_ffn_pipe_ns<16>(p, grid, s);
  }
}
