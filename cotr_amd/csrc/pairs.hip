// Pairs calls (api.hip cotr_encode_pairs): M distinct images, B index pairs.  Two copies frame the existing encode stages:
//  * pack: two images [3,256,256] NCHW -> one side-by-side slot [3,256,512] NCHW, the input the backbone stem reads.  An odd image
//    count leaves the last slot's right half zero (its features are computed and never read).
//  * gather: a pass's encoder input [Bc*512, 256] from the per-image input_proj rows.  The image region is slot-major - image m is half
//    m & 1 of slot m >> 1, [slots][512 tokens][256] exactly as input_proj writes it - so token (y, x) of pair b is row
//    (img >> 1) * 512 + y * 32 + (img & 1) * 16 + (x & 15) with img = x < 16 ? left[b] : right[b].
// Both are 16-byte loads and stores, one float4 per lane; the indices come in the kernel arguments (no device table, no host wait).
#include "common.h"

namespace {

// one float4 of a slot per thread: 128 float4 per 512-wide image row, 3 * 256 rows per slot
__global__ __launch_bounds__(256) void pack_pairs_kernel(const float* __restrict__ images, int M, int m0, float* __restrict__ out,
                                                         long n4) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const int x4 = (int)(i & 127);                  // float4 column of the 512-wide row
  const long row = i >> 7;                        // slot * 768 + c * 256 + y
  const int slot = (int)(row / 768), cy = (int)(row % 768);
  const int m = m0 + 2 * slot + (x4 >> 6);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (m < M) v = *reinterpret_cast<const f32x4*>(images + ((size_t)m * 768 + cy) * 256 + (x4 & 63) * 4);
  *reinterpret_cast<f32x4*>(out + (size_t)i * 4) = v;
}

// one float4 of a token row per thread: 64 float4 per row, 512 rows per pair
__global__ __launch_bounds__(256) void gather_pairs_kernel(const float* __restrict__ src, PairIdx idx, float* __restrict__ out, long n4) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const int c4 = (int)(i & 63);
  const long row = i >> 6;                        // pair * 512 + y * 32 + x
  const int b = (int)(row >> 9), t = (int)(row & 511), x = t & 31;
  const int m = x < 16 ? idx.left[b] : idx.right[b];
  const size_t srow = (size_t)(m >> 1) * 512 + (t & ~31) + (m & 1) * 16 + (x & 15);
  *reinterpret_cast<f32x4*>(out + (size_t)row * 256 + c4 * 4) = *reinterpret_cast<const f32x4*>(src + srow * 256 + c4 * 4);
}

}  // namespace

int launch_pack_pairs(const float* images, int M, int m0, int slots, float* out, hipStream_t s) {
  if (!images || !out || M <= 0 || slots <= 0 || m0 < 0 || m0 >= M || m0 + 2 * (slots - 1) >= M) return -1;
  const long n4 = (long)slots * 3 * 256 * 128;
  hipLaunchKernelGGL(pack_pairs_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, images, M, m0, out, n4);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

int launch_gather_pairs(const float* src, const PairIdx& idx, int nb, float* out, hipStream_t s) {
  if (!src || !out || nb <= 0 || nb > PAIR_IDX_MAX) return -1;
  const long n4 = (long)nb * 512 * 64;
  hipLaunchKernelGGL(gather_pairs_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, src, idx, out, n4);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}
