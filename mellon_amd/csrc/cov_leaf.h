// The per-leaf device arithmetic of the covariance kernels -- value, radial gradient factor g, second radial factor h and
// the tiled leaf dot product -- shared by cov_kernels.hip, cov_predict_deriv.hip, cov_grad.hip (one-program routes) and cov_block_deriv.hip
// (block-evaluated trees), so that every route evaluates a leaf with the same instructions.
#pragma once
#include "mln_internal.h"
#include "cov_rows.h"

namespace covtile { constexpr int TM = 64, TN = covrows::TN, DK = 16, PADT = 4; }
// Divisions by the length scale / by 3 are multiplications by the reciprocal (one rounding instead of
// a ~20-instruction fp64 divide per element): values differ from the reference's `x / ls` by <= 1 ulp.
static __device__ __forceinline__ double leaf_value(const DevLeaf& lf, double xx, double yy, double xy) {
  const double inv_ls = lf.alpha_inv_ls[1];
  if (lf.kind == MLN_K_LINEAR) return xy * inv_ls;          // cov.py:554
  // util.py:362-366: sq = xx - 2 xy + yy + 1e-12 ; dist = sqrt(max(sq, 0))
  double sq = xx - 2.0 * xy + yy + 1e-12;
  double dist = sqrt(fmax(sq, 0.0));
  switch (lf.kind) {
    case MLN_K_DISTANCE: return dist * inv_ls;              // util.py:366
    case MLN_K_MATERN32: {                                  // cov.py:64-65
      double r = 1.7320508075688772 * dist * inv_ls;
      return (r + 1.0) * exp(-r);
    }
    case MLN_K_MATERN52: {                                  // cov.py:159-160
      double r = 2.23606797749979 * dist * inv_ls;
      return (r + r * r * 0.3333333333333333 + 1.0) * exp(-r);
    }
    case MLN_K_EXPQUAD: {                                   // cov.py:257-258
      double r = dist * inv_ls;
      return exp(-0.5 * (r * r));
    }
    case MLN_K_EXPONENTIAL: {                               // cov.py:354-355
      double r = dist * inv_ls;
      return exp(-0.5 * r);
    }
    default: {                                              // RatQuad cov.py:455-456
      double r = dist * inv_ls;
      return pow(r * r / (2.0 * lf.alpha) + 1.0, -lf.alpha);
    }
  }
}

// Radial factor g of d leaf(x, y)/dx = g * (x - y)|dims (stationary leaves), the exact derivative of what
// leaf_value evaluates (denominator dist, 0 where the clamp of util.distance is active): the formulas of
// cov.py k_grad (cov.py:84-97,186-199,283-296,380-393,481-496) with util.distance_grad's +1e-12 dropped.
static __device__ __forceinline__ double leaf_grad_coeff(const DevLeaf& lf, double xx, double yy, double xy) {
  const double inv_ls = lf.alpha_inv_ls[1];
  const double sq = xx - 2.0 * xy + yy + 1e-12;
  const double dist = sqrt(fmax(sq, 0.0));
  const double inv = (sq > 0.0) ? 1.0 / dist : 0.0;
  switch (lf.kind) {
    case MLN_K_MATERN32: {
      const double f = 1.7320508075688772 * inv_ls, r = f * dist;
      return -f * r * exp(-r) * inv;
    }
    case MLN_K_MATERN52: {
      const double f = 2.23606797749979 * inv_ls, r = f * dist;
      return -0.3333333333333333 * exp(-r) * r * (r + 1.0) * f * inv;
    }
    case MLN_K_EXPQUAD: {
      const double r = dist * inv_ls;
      return -r * inv_ls * exp(-0.5 * (r * r)) * inv;
    }
    case MLN_K_EXPONENTIAL: {
      const double r = dist * inv_ls;
      return -0.5 * inv_ls * exp(-0.5 * r) * inv;
    }
    default: {
      const double r = dist * inv_ls, b = r * r / (2.0 * lf.alpha) + 1.0;
      return -r * inv_ls * pow(b, -lf.alpha - 1.0) * inv;
    }
  }
}

// acc[i][j] = sum_k x[row0+ty*4+i][dims[k]] * y[col0+tx*4+j][dims[k]] over one leaf's active dims
static __device__ __forceinline__ void leaf_dot(const DevCov& cov, const DevLeaf& lf, const double* __restrict__ x,
                                         int64_t n, const double* __restrict__ y, int64_t m, int d,
                                         int64_t row0, int64_t col0, double (*xs)[covtile::TM + covtile::PADT],
                                         double (*ys)[covtile::TN + covtile::PADT], double acc[4][4]) {
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
  for (int k0 = 0; k0 < lf.ndims; k0 += covtile::DK) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      int idx = tid + 256 * q;
      int r = idx >> 4, k = idx & 15;
      double vx = 0.0, vy = 0.0;
      if (k0 + k < lf.ndims) {
        int col = cov.dims[lf.dims_off + k0 + k];
        if (row0 + r < n) vx = x[(row0 + r) * (int64_t)d + col];
        if (col0 + r < m) vy = y[(col0 + r) * (int64_t)d + col];
      }
      xs[k][r] = vx;
      ys[k][r] = vy;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < covtile::DK; ++k) {
      double a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = xs[k][ty * 4 + i];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = ys[k][tx * 4 + j];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fma(a[i], b[j], acc[i][j]);
    }
  }
}

// Second radial factor h of a stationary leaf: Hessian = g I|dims + h (x - c)(x - c)^T|dims (see k_hess_coeff).
static __device__ __forceinline__ double leaf_hess_coeff(const DevLeaf& lf, double xx, double yy, double xy) {
  const double inv_ls = lf.alpha_inv_ls[1];
  const double sq = xx - 2.0 * xy + yy + 1e-12;
  if (!(sq > 0.0) || lf.kind == MLN_K_LINEAR) return 0.0;
  const double dist = sqrt(sq), il2 = inv_ls * inv_ls;
  switch (lf.kind) {
    case MLN_K_MATERN32: {                  // g = -f^2 e^{-f r}
      const double f = 1.7320508075688772 * inv_ls;
      return f * f * f * exp(-f * dist) / dist;
    }
    case MLN_K_MATERN52: {                  // g = -(f^2 / 3)(1 + f r) e^{-f r}
      const double f = 2.23606797749979 * inv_ls, f2 = f * f;
      return f2 * f2 * exp(-f * dist) * 0.3333333333333333;
    }
    case MLN_K_EXPQUAD: {                   // g = -k / ls^2
      const double r = dist * inv_ls;
      return exp(-0.5 * (r * r)) * il2 * il2;
    }
    case MLN_K_EXPONENTIAL: {               // g = -k / (2 ls r)
      const double e = exp(-0.5 * dist * inv_ls);
      return e * (0.25 * il2 / sq + 0.5 * inv_ls / (sq * dist));
    }
    default: {                              // RatQuad: g = -b^{-alpha-1} / ls^2
      const double r = dist * inv_ls, b = r * r / (2.0 * lf.alpha) + 1.0;
      return (lf.alpha + 1.0) / lf.alpha * pow(b, -lf.alpha - 2.0) * il2 * il2;
    }
  }
}

// value and radial gradient factor of one leaf.  exact_denominator = 0: distance_grad's
// delta / (dist + 1e-12) (k_grad); 1: the exact derivative of sqrt(max(sq, 0)), delta / dist (what
// autodiff of `_mean` gives), 0 where the clamp is active.
static __device__ __forceinline__ void leaf_value_grad(const DevLeaf& lf, double xx, double yy, double xy,
                                                int exact_denominator, double* k, double* g) {
  const double inv_ls = lf.alpha_inv_ls[1];
  if (lf.kind == MLN_K_LINEAR) { *k = xy * inv_ls; *g = inv_ls; return; }
  const double sq = xx - 2.0 * xy + yy + 1e-12;
  const double dist = sqrt(fmax(sq, 0.0));
  const double inv = exact_denominator ? ((sq > 0.0) ? 1.0 / dist : 0.0) : 1.0 / (dist + 1e-12);
  switch (lf.kind) {
    case MLN_K_MATERN32: {                                   // cov.py:84-97
      const double f = 1.7320508075688772 * inv_ls, r = f * dist, e = exp(-r);
      *k = (r + 1.0) * e;
      *g = -f * r * e * inv;
      break;
    }
    case MLN_K_MATERN52: {                                   // cov.py:186-199
      const double f = 2.23606797749979 * inv_ls, r = f * dist, e = exp(-r);
      *k = (r + r * r * 0.3333333333333333 + 1.0) * e;
      *g = -0.3333333333333333 * e * r * (r + 1.0) * f * inv;
      break;
    }
    case MLN_K_EXPQUAD: {                                    // cov.py:283-296
      const double r = dist * inv_ls, e = exp(-0.5 * (r * r));
      *k = e;
      *g = -r * inv_ls * e * inv;
      break;
    }
    case MLN_K_EXPONENTIAL: {                                // cov.py:380-393
      const double r = dist * inv_ls, e = exp(-0.5 * r);
      *k = e;
      *g = -0.5 * inv_ls * e * inv;
      break;
    }
    default: {                                               // RatQuad cov.py:481-496
      const double r = dist * inv_ls, b = r * r / (2.0 * lf.alpha) + 1.0;
      *k = pow(b, -lf.alpha);
      *g = -r * inv_ls * pow(b, -lf.alpha - 1.0) * inv;
    }
  }
}
