// The covariance program on one 64 x 64 tile, 4 x 4 outputs per thread (the layout of cov_kernels.hip): shared by the kernel
// matrix and the fused predictive mean (cov_kernels.hip) and by the single-leaf coefficient pass of the predictor gradient
// (cov_predict_deriv.hip).
#pragma once
#include "cov_program.h"
#include "cov_leaf.h"

// Evaluates the whole covariance program for this thread's 4x4 outputs into val.
template <bool SINGLE, bool GRADC = false>
__device__ __forceinline__ void cov_tile(const DevCov& cov, const double* __restrict__ x, int64_t n,
                                         const double* __restrict__ y, int64_t m, int d,
                                         const double* __restrict__ xx, const double* __restrict__ yy,
                                         int64_t row0, int64_t col0, double (*xs)[covtile::TM + covtile::PADT],
                                         double (*ys)[covtile::TN + covtile::PADT], double val[4][4]) {
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  double s1[4][4], s2[4][4];  // stack below the top (val is the top); max depth 3
  int sp = 0;
  const int ntok = SINGLE ? 1 : cov.n_toks;
  for (int t = 0; t < ntok; ++t) {
    const int op = SINGLE ? MLN_OP_LEAF : cov.tok_op[t];
    if (op == MLN_OP_LEAF || op == MLN_OP_CONST) {
      if (!SINGLE && sp > 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) { s2[i][j] = s1[i][j]; s1[i][j] = val[i][j]; }
      }
      if (op == MLN_OP_CONST) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) val[i][j] = cov.tok_val[t];
      } else {
        const int li = SINGLE ? 0 : cov.tok_leaf[t];
        const DevLeaf lf = cov.leaves[li];
        double acc[4][4];
        leaf_dot(cov, lf, x, n, y, m, d, row0, col0, xs, ys, acc);
        double xr[4], yr[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          int64_t r = row0 + ty * 4 + i;
          xr[i] = (r < n) ? xx[(int64_t)li * n + r] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          int64_t c = col0 + tx * 4 + j;
          yr[j] = (c < m) ? yy[(int64_t)li * m + c] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            val[i][j] = GRADC ? leaf_grad_coeff(lf, xr[i], yr[j], acc[i][j]) : leaf_value(lf, xr[i], yr[j], acc[i][j]);
      }
      ++sp;
    } else {
      // binary op: left = s1, right = val (top)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          double l = s1[i][j], r = val[i][j];
          val[i][j] = (op == MLN_OP_ADD) ? (l + r) : (op == MLN_OP_MUL) ? (l * r) : pow(l, r);
          s1[i][j] = s2[i][j];
        }
      --sp;
    }
  }
}
