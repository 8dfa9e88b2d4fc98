// (included by cov_rows_*.hip, one translation unit per kernel kind: 30 instantiations in one unit take ~10 min)
// Kernel-matrix pass of the fit in the persistent-row form of rows_pipeline.h: K = cov(x, xu) for one stationary leaf
// over all d <= 64 columns (reference: util.py:351-366 `distance`, cov.py k() of Matern32/52, ExpQuad, Exponential).
// sqrt and exp are the straight-line code of cov_epilogue.h instead of the library routines with their special-case selects.
// (The product of two leaves: kernel_rows_prod_impl.h, which also uses surrogate_bits from here.)
#pragma once
#include "rows_pipeline.h"

namespace {
using covrows::TN;

// the 32-bit copy: the fixed-point number round(v 2^32), 1 stored as 2^32 - 1 -- see mln_internal.h.  (The rows kernels
// only ever write this format -- every kind they handle is bounded by 1; an fp32 copy, MELLON_AMD_SURROGATE=float,
// takes the tiled kernel.  A run-time choice between the two cost 5 instead of 3 instructions per element here.)
// No conversion instruction: v + 2^20 has an ulp of 2^-32, so the low word of that double IS round(v 2^32) (to nearest
// even); v is clamped to 1 - 2^-32 first, where the sum would carry into bit 32.
__device__ __forceinline__ float surrogate_bits(double v, int) {
  return __uint_as_float((unsigned)__double2loint(fmin(v, 0x1.fffffffep-1) + 0x1p20));
}

// covariance value from the pre-scaled norms (cov_epilogue.h): xs = c2 (|x|^2 + 1e-12), ys = c2 |y|^2, m2 = -2 c2
template <int KIND>
__device__ __forceinline__ double leaf_value_k(double m2, double xs, double ys, double xy) {
  return covepi::leaf_value_s<KIND>(fmax(fma(m2, xy, xs) + ys, 1e-300));
}

// The tile walk and the stores; `value(r, xy, s)` is the matrix element of the lane's row r from its dot
// product and the side values s[] of its centre.  FAST tiles (interior rows, full tile, no diagonal term) are stored
// branch-free: a wave-uniform base per tile and column group (SGPR pair, scalar arithmetic) + ONE 32-bit byte offset per
// lane and row, shared by all 16 column positions (and, halved, by the 32-bit copy) -- no vector instruction per store.
// The other tiles clamp rows and columns, add the diagonal term and zero the pad columns of the leading dimension.
template <bool HAS32, int KSTEPS, int EPI_VALU, class Value>
__device__ __forceinline__ void kernel_matrix_rows_body(const double* __restrict__ x, int64_t n, const double* __restrict__ y,
                                                        int64_t m, int d, const double* __restrict__ yy, double c2,
                                                        double* __restrict__ out, int64_t ldo, double add_diag,
                                                        float* __restrict__ out32, int q32, Value&& value) {
  constexpr int NSIDE = 1;
  const rowspipe::Lane L = rowspipe::lane();
  double* const out_wg = out + (int64_t)blockIdx.x * 128 * ldo;
  float* const out32_wg = HAS32 ? out32 + (int64_t)blockIdx.x * 128 * ldo : nullptr;
  unsigned lrowb[4], lrowb32[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    lrowb[r] = ((unsigned)(L.wave * 16 + L.lk + 4 * r) * (unsigned)ldo + (unsigned)L.li) * 8u;
    lrowb32[r] = lrowb[r] >> 1;
  }
  auto epilogue = [&](const v4d_t (&cur)[4], rowspipe::SideTile side, int64_t col0, auto fast_tag) {
    if (decltype(fast_tag)::value) {
      char* const ob = (char*)(out_wg + col0);
      char* const ob32 = HAS32 ? (char*)(out32_wg + col0) : nullptr;
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        double s[NSIDE];
#pragma unroll
        for (int k = 0; k < NSIDE; ++k) s[k] = side(k, tt);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double v = value(r, cur[tt][r], s);
          *(double*)(ob + 128 * tt + lrowb[r]) = v;
          if (HAS32) *(float*)(ob32 + 64 * tt + lrowb32[r]) = surrogate_bits(v, q32);
        }
      }
    } else {
#pragma unroll
      for (int tt = 0; tt < 4; ++tt) {
        const int64_t c = col0 + 16 * tt + L.li;
        double s[NSIDE];
#pragma unroll
        for (int k = 0; k < NSIDE; ++k) s[k] = side(k, tt);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t row = L.row(r);
          if (row < n && c < ldo) {
            const double v = (c < m) ? value(r, cur[tt][r], s) + ((row == c) ? add_diag : 0.0) : 0.0;
            out[row * ldo + c] = v;
            if (HAS32) out32[row * ldo + c] = surrogate_bits(v, q32);
          }
        }
      }
    }
  };
  const int64_t ntiles = (ldo + TN - 1) / TN;   // covers the pad columns of the leading dimension
  const bool interior_rows = (int64_t)blockIdx.x * 128 + 128 <= n;
  const int64_t n_fast = (interior_rows && add_diag == 0.0) ? (m / TN) : 0;   // full tiles of interior rows
  rowspipe::rows_pipeline<KSTEPS, false, false, true, EPI_VALU>(x, n, y, d, yy, nullptr, c2, 0.0, ntiles, n_fast, epilogue);
}

template <int KIND, bool HAS32, int KSTEPS>
__global__ __launch_bounds__(512) void k_kernel_matrix_rows(DevCov cov, const double* __restrict__ x, int64_t n,
                                                            const double* __restrict__ y, int64_t m, int d,
                                                            const double* __restrict__ xx,
                                                            const double* __restrict__ yy,
                                                            double* __restrict__ out, int64_t ldo, double add_diag,
                                                            float* __restrict__ out32, int q32) {
  const double c2 = covepi::sq_scale<KIND>(cov.leaves[0]), m2 = -2.0 * c2;
  const rowspipe::Lane L = rowspipe::lane();
  double xr[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) xr[r] = (L.row(r) < n) ? c2 * (xx[L.row(r)] + 1e-12) : 0.0;   // util.py:362-366's + 1e-12 rides with the row norm
  kernel_matrix_rows_body<HAS32, KSTEPS, (HAS32 ? 32 : 29) * 16 + 8>(
      x, n, y, m, d, yy, c2, out, ldo, add_diag, out32, q32,
      [&](int r, double xy, const double* s) { return leaf_value_k<KIND>(m2, xr[r], s[rowspipe::SIDE_NORM], xy); });
}

}  // namespace

// (PROD = true, the product kernel: kernel_rows_prod_impl.h)
template <int KIND, bool PROD>
int launch_kernel_matrix_rows_kind(mln_ctx* ctx, const DevCov& cov, const double* x, int64_t n, const double* y, int64_t m,
                                   int d, const double* xx, const double* yy, double* out, int64_t ldo, double add_diag,
                                   float* out32, int q32) {
  static_assert(!PROD, "the product kernels are launched from kernel_rows_prod_impl.h");
  const dim3 grid((unsigned)((n + 127) / 128)), block(512);
#define MLN_KM_ROWS2(KS)                                                                                              \
  if (out32) hipLaunchKernelGGL((k_kernel_matrix_rows<KIND, true, KS>), grid, block, 0, ctx->stream, cov, x, n, y, m, d, \
                                xx, yy, out, ldo, add_diag, out32, q32);                                             \
  else hipLaunchKernelGGL((k_kernel_matrix_rows<KIND, false, KS>), grid, block, 0, ctx->stream, cov, x, n, y, m, d, xx,  \
                          yy, out, ldo, add_diag, out32, q32);
  if (d <= 32) { MLN_KM_ROWS2(8) }
  else if (d <= 52) { MLN_KM_ROWS2(13) }
  else { MLN_KM_ROWS2(16) }
#undef MLN_KM_ROWS2
  MLN_HIP(ctx, hipGetLastError());
  return MLN_OK;
}
