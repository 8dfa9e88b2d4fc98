// The special functions of the dimensionality likelihood, shared by its single pass (dimensionality.hip) and its batched
// pass (dim_objective_batch.hip).
#pragma once
#include <hip/hip_runtime.h>

// lnGamma, digamma and trigamma for x >= 1 (the argument D / 2 + 1 of the likelihood), sharing one shift: the recurrences up
// to x >= 6, then the asymptotic series (Stirling's through x^-13, digamma's through x^-14, trigamma's through x^-15: the
// first omitted term is below 1e-13 at x = 6).  The device library's lgamma costs more than a hundred registers in the
// objective's loop; these are a few dozen instructions.
template <bool TRI>
__device__ __forceinline__ void gamma_fns(double x, double& lg, double& ps, double& tp) {
  double prod = 1.0, rps = 0.0, rtp = 0.0;
  while (x < 6.0) {
    prod *= x;
    const double ix = 1.0 / x;
    rps -= ix;
    if (TRI) rtp = fma(ix, ix, rtp);
    x += 1.0;
  }
  const double ix = 1.0 / x, i2 = ix * ix, lx = log(x);
  const double st = ix * (1.0 / 12 - i2 * (1.0 / 360 - i2 * (1.0 / 1260 - i2 * (1.0 / 1680 - i2 * (1.0 / 1188 - i2 * (691.0 / 360360 - i2 / 156))))));
  lg = (x - 0.5) * lx - x + 0.91893853320467274178 + st - log(prod);      // 0.9189... = log(2 pi) / 2
  const double sd = i2 * (1.0 / 12 - i2 * (1.0 / 120 - i2 * (1.0 / 252 - i2 * (1.0 / 240 - i2 * (1.0 / 132 - i2 * (691.0 / 32760 - i2 / 12))))));
  ps = rps + lx - 0.5 * ix - sd;
  if (TRI) {
    const double s3 = ix * i2 * (1.0 / 6 - i2 * (1.0 / 30 - i2 * (1.0 / 42 - i2 * (1.0 / 30 - i2 * (5.0 / 66 - i2 * (691.0 / 2730 - i2 * 7.0 / 6))))));
    tp = rtp + ix + 0.5 * i2 + s3;
  } else {
    tp = 0.0;
  }
}
