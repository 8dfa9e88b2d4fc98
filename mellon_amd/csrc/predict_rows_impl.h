// (included by predict_rows_*.hip and predict_rows_prod_*.hip, one translation unit per kernel kind and family: the
// fifteen instantiations in one unit took 25 min)
// Fused predictive mean (reference: conditional.py:899-906 `_mean`, one output column) in the persistent-row form of
// rows_pipeline.h: the epilogue of a tile multiplies each covariance value by its centre's weight and adds it to the
// row sums; the n' x m matrix never exists.
//   * one stationary leaf over all d <= 64 columns;
//   * the time-sensitive product  k(ls, active_dims=:-1) * k(ls_time, active_dims=-1)  (reference: parameters.py:641-644
//     builds it; PredictorTime.mean, base_predictor.py:872-948): the epilogue evaluates BOTH leaves per element -- the
//     state leaf from the MFMA's dot product, the time leaf from the two time stamps -- with one exponential for the two
//     (cov_epilogue.h).
// The library sqrt / exp cost ~100 instructions per element and leaf here; cov_epilogue.h replaces them.
#pragma once
#include "rows_pipeline.h"

namespace {
using covrows::TN;

// scaled squared distance -> covariance value (cov_epilogue.h); RatQuad, the one kind without an exponential, through pow
template <int KIND>
__device__ __forceinline__ double value_of(double s, double alpha) {
  if (KIND == MLN_K_RATQUAD) return pow(fmax(s, 0.0) + 1.0, -alpha);       // cov.py:453-457, s = (dist / ls)^2 / (2 alpha)
  return covepi::leaf_value_s<KIND>(fmax(s, 1e-300));
}

// The tile walk, the row sums and their reduction for both kernels; `value(r, xy, s)` is the covariance of the lane's
// row r and a centre from their dot product and the centre's side values s[].
template <bool TIME, int KSTEPS, int EPI_VALU, class Value>
__device__ __forceinline__ void predict_mean_rows_body(const double* __restrict__ x, int64_t n, const double* __restrict__ y,
                                                       int64_t m, int d, const double* __restrict__ yy,
                                                       const double* __restrict__ w, double c2, double c1, double mu,
                                                       double* __restrict__ out, Value&& value) {
  constexpr int NSIDE = TIME ? 3 : 2;
  const rowspipe::Lane L = rowspipe::lane();
  double part[4] = {0.0, 0.0, 0.0, 0.0};
  auto epilogue = [&](const v4d_t (&cur)[4], rowspipe::SideTile side, int64_t, auto) {
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
      double s[NSIDE];
#pragma unroll
      for (int k = 0; k < NSIDE; ++k) s[k] = side(k, tt);
#pragma unroll
      for (int r = 0; r < 4; ++r) part[r] = fma(value(r, cur[tt][r], s), s[rowspipe::side_weight(TIME)], part[r]);
    }
  };
  const int64_t ntiles = (m + TN - 1) / TN;
  rowspipe::rows_pipeline<KSTEPS, TIME, true, false, EPI_VALU>(x, n, y, d, yy, w, c2, c1, ntiles, ntiles, epilogue);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double s_ = part[r];
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) s_ += __shfl_xor(s_, off, 64);
    if (L.li == 0 && L.row(r) < n) out[L.row(r)] = mu + s_;
  }
}

template <int KIND, int KSTEPS>
__global__ __launch_bounds__(512) void k_predict_mean_rows(DevCov cov, const double* __restrict__ x, int64_t n,
                                                           const double* __restrict__ y, int64_t m, int d,
                                                           const double* __restrict__ xx,
                                                           const double* __restrict__ yy,
                                                           const double* __restrict__ w, double mu,
                                                           double* __restrict__ out) {
  const double c2 = covepi::sq_scale<KIND>(cov.leaves[0]), m2 = -2.0 * c2, alpha = cov.leaves[0].alpha;
  const rowspipe::Lane L = rowspipe::lane();
  double xr[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) xr[r] = (L.row(r) < n) ? c2 * (xx[L.row(r)] + 1e-12) : 0.0;
  // (RatQuad's library pow: the interleave is left to the scheduler's own devices)
  predict_mean_rows_body<false, KSTEPS, (KIND == MLN_K_RATQUAD) ? 0 : 30 * 16 + 8>(
      x, n, y, m, d, yy, w, c2, 0.0, mu, out, [&](int r, double xy, const double* s) {
        return value_of<KIND>(fma(m2, xy, xr[r]) + s[rowspipe::SIDE_NORM], alpha);
      });
}

// The product: column d - 1 of x and y is the time stamp, xx and yy are |x_state|^2 (leaf 0's norms).
template <int KIND, int KSTEPS>
__global__ __launch_bounds__(512) void k_predict_mean_rows_prod(DevCov cov, const double* __restrict__ x, int64_t n,
                                                                const double* __restrict__ y, int64_t m, int d,
                                                                const double* __restrict__ xx,
                                                                const double* __restrict__ yy,
                                                                const double* __restrict__ w, double mu,
                                                                double* __restrict__ out) {
  // the time leaf's squared distance directly from the two pre-scaled stamps: see k_kernel_matrix_rows_prod (kernel_rows_prod_impl.h)
  const double c20 = covepi::sq_scale<KIND>(cov.leaves[0]), m20 = -2.0 * c20;
  const double c21 = covepi::sq_scale<KIND>(cov.leaves[1]), c1 = sqrt(c21), eps1 = c21 * 1e-12;
  const rowspipe::Lane L = rowspipe::lane();
  double xr[4], xt[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    xr[r] = (L.row(r) < n) ? c20 * (xx[L.row(r)] + 1e-12) : 0.0;
    xt[r] = (L.row(r) < n) ? c1 * x[L.row(r) * d + d - 1] : 0.0;
  }
  predict_mean_rows_body<true, KSTEPS, 40 * 16 + 12>(
      x, n, y, m, d, yy, w, c20, c1, mu, out, [&](int r, double xy, const double* s) {
        const double yc = s[rowspipe::SIDE_NORM], tc = s[rowspipe::SIDE_TIME];
        const double dt = xt[r] - tc;
        return covepi::leaf_product_s<KIND>(fmax(fma(m20, xy, xr[r]) + yc, 1e-300), fma(dt, dt, eps1));
      });
}

}  // namespace

// PROD: the product kernel, whose operand columns are the d - 1 state columns
template <int KIND, bool PROD>
int launch_predict_mean_rows_kind(mln_ctx* ctx, const DevCov& cov, const double* x, int64_t n, const double* y, int64_t m,
                                  int d, const double* xx, const double* yy, const double* w, double mu, double* out) {
  const dim3 grid((unsigned)((n + 127) / 128)), block(512);
  const int ds = PROD ? d - 1 : d;
#define MLN_PM_ROWS2(KS)                                                                                                \
  if constexpr (PROD) hipLaunchKernelGGL((k_predict_mean_rows_prod<KIND, KS>), grid, block, 0, ctx->stream, cov, x, n, y, \
                                         m, d, xx, yy, w, mu, out);                                                     \
  else hipLaunchKernelGGL((k_predict_mean_rows<KIND, KS>), grid, block, 0, ctx->stream, cov, x, n, y, m, d, xx, yy, w,    \
                          mu, out);
  if (ds <= 32) { MLN_PM_ROWS2(8) }
  else if (ds <= 52) { MLN_PM_ROWS2(13) }
  else { MLN_PM_ROWS2(16) }
#undef MLN_PM_ROWS2
  MLN_HIP(ctx, hipGetLastError());
  return MLN_OK;
}
