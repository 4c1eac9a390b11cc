// The rotation step of the Gauss-Newton refits (pnp.hip: absolute pose, essential.hip: relative pose).  Rule in DESIGN.md 3h-4.
// Included by translation units compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// R <- exp([w]x) R by Rodrigues' formula; sin th / th = 1 and (1 - cos th) / th^2 = 1/2 below 1e-8
__device__ inline void rodrigues_rotate(const double* w, double* R) {
  const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2], th = sqrt(th2);
  const double a = th > 1e-8 ? sin(th) / th : 1.0, b = th > 1e-8 ? (1.0 - cos(th)) / th2 : 0.5;
  const double W[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
  double E[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double ww = (W[i * 3] * W[j] + W[i * 3 + 1] * W[3 + j]) + W[i * 3 + 2] * W[6 + j];
      E[i * 3 + j] = ((i == j ? 1.0 : 0.0) + a * W[i * 3 + j]) + b * ww;
    }
  double out[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) out[i * 3 + j] = (E[i * 3] * R[j] + E[i * 3 + 1] * R[3 + j]) + E[i * 3 + 2] * R[6 + j];
  for (int i = 0; i < 9; ++i) R[i] = out[i];
}
