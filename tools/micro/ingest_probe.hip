// Micro-benchmark: does a CU take in more bytes per second with two resident workgroups than with one?  gfx950.
// Every workgroup (256 threads) streams the per-workgroup bytes of the decoder's fused attention launch (attention_kernel<4, 2, true>
// at one pair x 1000 queries): K_h and V_h of its head (512 keys x 32 floats each, rows 2 KB apart as in the K/V projection output,
// 128 KB), Wq_h (32 rows x 256, 32 KB), the head's 32 columns of W_out (256 rows x 32 floats, 32 KB) and 32 query rows (32 KB) -
// 224 KB, L2-warm.  256 workgroups = one per CU; 512 = two per CU (the 16-query-tile decoder form would run 504).
//   hipcc --offload-arch=gfx950 -O3 -o tools/micro/ingest_probe.exe tools/micro/ingest_probe.hip && tools/micro/ingest_probe.exe
#include <hip/hip_runtime.h>
#include <stdio.h>

constexpr int ROWS = 1024;   // query rows of x (1000 rounded up); query tile t reads rows (32 t .. 32 t + 31) mod ROWS

__global__ __launch_bounds__(256) void ingest(const float4* __restrict__ kv, const float4* __restrict__ wq, const float4* __restrict__ wo,
                                              const float4* __restrict__ x, float* __restrict__ sink) {
  const int t = threadIdx.x, head = blockIdx.x & 7, qtile = blockIdx.x >> 3;
  float4 acc = {0.f, 0.f, 0.f, 0.f};
  // K_h / V_h: kv is [512 keys][512 floats] = [512][128 float4]; head h's K at float4 column 8 h, its V at 64 + 8 h (8 float4 each)
#pragma unroll 8
  for (int i = t; i < 512 * 16; i += 256) {
    const int key = i >> 4, c = i & 15;
    const float4 a = kv[key * 128 + (c < 8 ? 8 * head + c : 64 + 8 * head + c - 8)];
    acc.x += a.x; acc.y += a.y; acc.z += a.z; acc.w += a.w;
  }
  // Wq_h: rows 32 h .. 32 h + 31 of [256][64 float4]
#pragma unroll 8
  for (int i = t; i < 32 * 64; i += 256) {
    const float4 a = wq[(32 * head + (i >> 6)) * 64 + (i & 63)];
    acc.x += a.x; acc.y += a.y; acc.z += a.z; acc.w += a.w;
  }
  // W_out: every row, float4 columns 8 h .. 8 h + 7
#pragma unroll 8
  for (int i = t; i < 256 * 8; i += 256) {
    const float4 a = wo[(i >> 3) * 64 + 8 * head + (i & 7)];
    acc.x += a.x; acc.y += a.y; acc.z += a.z; acc.w += a.w;
  }
  // 32 query rows of [ROWS][64 float4]
#pragma unroll 8
  for (int i = t; i < 32 * 64; i += 256) {
    const float4 a = x[((qtile * 32 + (i >> 6)) % ROWS) * 64 + (i & 63)];
    acc.x += a.x; acc.y += a.y; acc.z += a.z; acc.w += a.w;
  }
  const float s = acc.x + acc.y + acc.z + acc.w;
  if (s == 12345.f) sink[blockIdx.x * 256 + t] = s;   // never true for the zero-filled inputs; keeps the loads
}

int main() {
  float *kv, *wq, *wo, *x, *sink;
  (void)hipMalloc(&kv, 512 * 512 * 4); (void)hipMalloc(&wq, 256 * 256 * 4); (void)hipMalloc(&wo, 256 * 256 * 4);
  (void)hipMalloc(&x, ROWS * 256 * 4); (void)hipMalloc(&sink, 1024 * 256 * 4);
  (void)hipMemset(kv, 0, 512 * 512 * 4); (void)hipMemset(wq, 0, 256 * 256 * 4); (void)hipMemset(wo, 0, 256 * 256 * 4);
  (void)hipMemset(x, 0, ROWS * 256 * 4);
  int cus = 0;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0);
  hipEvent_t a, b;
  (void)hipEventCreate(&a); (void)hipEventCreate(&b);
  const double bytes_wg = (128 + 32 + 32 + 32) * 1024.0;
  for (int wgs : {256, 512, 256, 512}) {
    for (int w = 0; w < 20; ++w) hipLaunchKernelGGL(ingest, dim3(wgs), dim3(256), 0, 0, (const float4*)kv, (const float4*)wq, (const float4*)wo, (const float4*)x, sink);
    float best = 1e9f, sum = 0.f;
    const int N = 50;
    for (int r = 0; r < N; ++r) {
      (void)hipEventRecord(a, 0);
      hipLaunchKernelGGL(ingest, dim3(wgs), dim3(256), 0, 0, (const float4*)kv, (const float4*)wq, (const float4*)wo, (const float4*)x, sink);
      (void)hipEventRecord(b, 0);
      (void)hipEventSynchronize(b);
      float ms;
      (void)hipEventElapsedTime(&ms, a, b);
      best = ms < best ? ms : best;
      sum += ms;
    }
    const double us = best * 1e3, per_cu = bytes_wg * wgs / cus;
    printf("%3d workgroups (%.1f per CU): best %6.2f us, mean %6.2f us  %7.1f KB per CU  %6.1f GB/s per CU  %6.1f TB/s chip\n", wgs,
           (double)wgs / cus, us, sum * 1e3 / N, per_cu / 1024, per_cu / us * 1e-3, bytes_wg * wgs / us * 1e-6);
  }
  return hipGetLastError() == hipSuccess ? 0 : 1;
}
