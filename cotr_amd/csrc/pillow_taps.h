// Pillow's BILINEAR coefficient rule (precompute_coeffs of src/libImaging/Resample.c) for one output index, box = [0, in_size):
// the triangle filter's support scales with the down-scale factor, the taps are the input samples lo .. lo + n - 1 inside it,
// and a tap's weight is tri() at its distance from the centre divided by the sum of all of them.  Everything in double, in
// Pillow's order of operations: include only from files compiled with -ffp-contract=off (crop_resize.hip quantises the weights
// to 8-bit coefficients, dense_post.hip uses them as they are).
#pragma once

__device__ __forceinline__ double tri(double x) {
  if (x < 0.0) x = -x;
  return x < 1.0 ? 1.0 - x : 0.0;
}

// taps of output index xx when resizing in_size samples to out_size samples: first tap, tap count, centre, 1 / filterscale, weight sum
struct Taps {
  int lo, n;
  double center, ss, ww;
};

__device__ __forceinline__ Taps taps_for(int in_size, int out_size, int xx) {
  Taps t;
  const double scale = (double)in_size / (double)out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;
  t.ss = 1.0 / filterscale;
  t.center = ((double)xx + 0.5) * scale;
  int lo = (int)(t.center - support + 0.5);
  if (lo < 0) lo = 0;
  int hi = (int)(t.center + support + 0.5);
  if (hi > in_size) hi = in_size;
  t.lo = lo;
  t.n = hi - lo;
  t.ww = 0.0;
  for (int x = 0; x < t.n; ++x) t.ww += tri(((double)(x + lo) - t.center + 0.5) * t.ss);
  return t;
}

__device__ __forceinline__ double tap_weight(const Taps& t, int x) {
  double w = tri(((double)(x + t.lo) - t.center + 0.5) * t.ss);
  if (t.ww != 0.0) w /= t.ww;
  return w;
}
