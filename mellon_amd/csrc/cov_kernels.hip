// Pairwise-distance + covariance tiles (reference: mellon/util.py:351-366 `distance`,
// mellon/cov.py k() of Matern32/52, ExpQuad, Exponential, RatQuad, Linear and
// mellon/base_cov.py:301-453 Add/Mul/Pow), fp64, gfx950.
//
// Layout: 64 cells x 64 centres per 256-thread workgroup, 4x4 outputs per thread.  The cell and
// centre tiles are staged k-major in LDS in chunks of 16 active dims (coalesced 128-B row reads),
// the x.y dot product is an fp64 FMA chain in registers, and the sqrt/exp epilogue runs on the
// same registers -- the n x m distance matrix never exists in HBM.  d <= 51 is too skinny for
// the fp64 MFMA (same rate as v_fma_f64 on gfx950) to pay, so this is a VALU kernel.
#include <cstdlib>

#include "mln_internal.h"
#include "rowmin_f16.h"
#include "rowmin_wide.h"
#include "cov_tile.h"
#include "cov_rows.h"
#include "mln_options.h"

namespace {

constexpr int TM = covtile::TM, TN = covtile::TN, DK = covtile::DK, PADT = covtile::PADT;
constexpr int NNS = covrows::NNS;

template <bool SINGLE>
__global__ __launch_bounds__(256) void k_kernel_matrix(DevCov cov, const double* __restrict__ x, int64_t n,
                                                       const double* __restrict__ y, int64_t m, int d,
                                                       const double* __restrict__ xx,
                                                       const double* __restrict__ yy,
                                                       double* __restrict__ out, int64_t ldo,
                                                       double add_diag, int64_t tiles_n,
                                                       float* __restrict__ out32, int q32) {
  __shared__ double xs[DK][TM + PADT];
  __shared__ double ys[DK][TN + PADT];
  const int64_t bid = blockIdx.x;
  const int64_t row0 = (bid / tiles_n) * TM, col0 = (bid % tiles_n) * TN;
  double val[4][4];
  cov_tile<SINGLE>(cov, x, n, y, m, d, xx, yy, row0, col0, xs, ys, val);
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int64_t r = row0 + ty * 4 + i;
    if (r >= n) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int64_t c = col0 + tx * 4 + j;
      const double v = (c < m) ? val[i][j] + ((r == c) ? add_diag : 0.0) : 0.0;
      if (c < ldo) {   // pad columns of the leading dimension stay zero
        out[r * ldo + c] = v;
        if (out32) out32[r * ldo + c] = mln_surrogate_bits(v, q32);   // 32-bit copy for the warm-up passes of the MAP solve
      }
    }
  }
}

// Single-leaf kernel matrix with the x.y dot products on the matrix cores: for one leaf over d contiguous
// columns the dot product is a plain (64 x d) x (d x 64) GEMM tile.  v_mfma_f64_16x16x4 with both operands
// read straight from global memory / L1 in the instruction's own layout (A[m = li][k = lk], B[k = lk][n = li];
// a tile of x or y is <= 26 KB and is re-read from L1 by the four waves).  Wave w owns rows 16 w .. 16 w + 15
// of the 64 x 64 tile (4 accumulators); the sqrt/exp epilogue and the fp64 (+ optional fp32) stores run on
// the accumulator layout D[row = lk + 4 reg][col = li].  Measured at 1e6 x 5000 x 50: 32 ms against 35 ms for
// the LDS-tiled VALU kernel above (PMC: VALU ~50 % busy on ~130 instructions per element, matrix pipe 20 %);
// staging this one-tile-per-workgroup form through LDS (38 ms) and hand-written sqrt/exp (no change) were
// tried and dropped; large shapes use k_kernel_matrix_rows below, which overlaps the matrix pipe with the
// epilogue inside each wave (27 ms).

__global__ __launch_bounds__(256) void k_kernel_matrix_mfma(DevCov cov, const double* __restrict__ x, int64_t n,
                                                            const double* __restrict__ y, int64_t m, int d,
                                                            const double* __restrict__ xx,
                                                            const double* __restrict__ yy,
                                                            double* __restrict__ out, int64_t ldo, double add_diag,
                                                            int64_t tiles_n, float* __restrict__ out32, int q32) {
  const DevLeaf lf = cov.leaves[0];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
  const int64_t bid = blockIdx.x;
  const int64_t row0 = (bid / tiles_n) * TM + wave * 16, col0 = (bid % tiles_n) * TN;
  // operand rows (clamped: loads stay unconditional, invalid rows / columns are never stored)
  const int64_t ar = (row0 + li < n) ? row0 + li : n - 1;
  const double* __restrict__ xa = x + ar * d;
  const double* yb[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int64_t c = col0 + 16 * t + li;
    yb[t] = y + ((c < m) ? c : m - 1) * d;
  }
  v4d_t acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = v4d_t{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < d; k0 += 4) {
    const int k = k0 + lk;
    const int kc = (k < d) ? k : d - 1;
    const double mask = (k < d) ? 1.0 : 0.0;
    const double a = xa[kc] * mask;
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, yb[t][kc], acc[t], 0, 0, 0);
  }
  double xr[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t row = row0 + lk + 4 * r;
    xr[r] = (row < n) ? xx[row] : 0.0;
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int64_t c = col0 + 16 * t + li;
    const double yc = (c < m) ? yy[c] : 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = row0 + lk + 4 * r;
      if (row < n && c < ldo) {   // pad columns of the leading dimension stay zero
        const double v = (c < m) ? leaf_value(lf, xr[r], yc, acc[t][r]) + ((row == c) ? add_diag : 0.0) : 0.0;
        out[row * ldo + c] = v;
        if (out32) out32[row * ldo + c] = mln_surrogate_bits(v, q32);
      }
    }
  }
}

// mean_i = mu + sum_j cov(x_i, y_j) w_j   (conditional.py:899-906); K never leaves registers.
template <bool SINGLE>
__global__ __launch_bounds__(256) void k_predict_mean1(DevCov cov, const double* __restrict__ x, int64_t n,
                                                       const double* __restrict__ y, int64_t m, int d,
                                                       const double* __restrict__ xx,
                                                       const double* __restrict__ yy,
                                                       const double* __restrict__ w, double mu,
                                                       double* __restrict__ out) {
  __shared__ double xs[DK][TM + PADT];
  __shared__ double ys[DK][TN + PADT];
  __shared__ double red[TM][17];
  const int64_t row0 = (int64_t)blockIdx.x * TM;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  double part[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t col0 = 0; col0 < m; col0 += TN) {
    double val[4][4];
    cov_tile<SINGLE>(cov, x, n, y, m, d, xx, yy, row0, col0, xs, ys, val);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int64_t c = col0 + tx * 4 + j;
      double wj = (c < m) ? w[c] : 0.0;
#pragma unroll
      for (int i = 0; i < 4; ++i) part[i] = fma(val[i][j], wj, part[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) red[ty * 4 + i][tx] = part[i];
  __syncthreads();
  if (threadIdx.x < TM) {
    double s = 0.0;
#pragma unroll
    for (int t = 0; t < 16; ++t) s += red[threadIdx.x][t];
    int64_t r = row0 + threadIdx.x;
    if (r < n) out[r] = mu + s;
  }
}

// Fused predictive mean on the matrix cores (single leaf over all d columns, one output): the tile scheme of
// k_kernel_matrix_mfma, but a wave keeps its 16 rows and walks ALL centre tiles, multiplying each covariance
// value by its weight and summing along the row -- the n' x m matrix never exists (conditional.py:899-906).
__global__ __launch_bounds__(256) void k_predict_mean_mfma(DevCov cov, const double* __restrict__ x, int64_t n,
                                                           const double* __restrict__ y, int64_t m, int d,
                                                           const double* __restrict__ xx,
                                                           const double* __restrict__ yy,
                                                           const double* __restrict__ w, double mu,
                                                           double* __restrict__ out) {
  const DevLeaf lf = cov.leaves[0];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * TM + wave * 16;
  const int64_t ar = (row0 + li < n) ? row0 + li : n - 1;
  const double* __restrict__ xa = x + ar * d;
  double xr[4], part[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t row = row0 + lk + 4 * r;
    xr[r] = (row < n) ? xx[row] : 0.0;
    part[r] = 0.0;
  }
  for (int64_t col0 = 0; col0 < m; col0 += TN) {
    const double* yb[4];
    double yc[4], wc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int64_t c = col0 + 16 * t + li;
      const int64_t cc = (c < m) ? c : m - 1;
      yb[t] = y + cc * d;
      yc[t] = yy[cc];
      wc[t] = (c < m) ? w[cc] : 0.0;
    }
    v4d_t acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = v4d_t{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < d; k0 += 4) {
      const int k = k0 + lk;
      const int kc = (k < d) ? k : d - 1;
      const double mask = (k < d) ? 1.0 : 0.0;
      const double a = xa[kc] * mask;
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, yb[t][kc], acc[t], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) part[r] = fma(leaf_value(lf, xr[r], yc[t], acc[t][r]), wc[t], part[r]);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double s_ = part[r];
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) s_ += __shfl_xor(s_, off, 64);   // over the 16 columns (li) of a row
    const int64_t row = row0 + lk + 4 * r;
    if (li == 0 && row < n) out[row] = mu + s_;
  }
}

// xx[leaf][i] = sum over the leaf's active dims of x_i^2   (util.py:362).  Eight lanes per row: a wave's load covers eight
// consecutive rows (3.2 KB of consecutive lines at d = 50) instead of 64 addresses d doubles apart -- one lane per row
// read the 0.4 GB of C3's cells at 0.47 TB/s (0.85 ms per fit).
__global__ __launch_bounds__(256) void k_row_sqnorms(DevCov cov, const double* __restrict__ x, int64_t n, int d,
                                                     double* __restrict__ xx) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 3;
  const int q = threadIdx.x & 7;
  const bool ok = i < n;
  const double* row = x + (ok ? i : 0) * (int64_t)d;
  for (int l = 0; l < cov.n_leaves; ++l) {
    const DevLeaf lf = cov.leaves[l];
    double s = 0.0;
    for (int k = q; k < lf.ndims; k += 8) {
      const double v = row[cov.dims[lf.dims_off + k]];
      s = fma(v, v, s);
    }
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    if (ok && q == 0) xx[(int64_t)l * n + i] = s;
  }
}


// The search compares |x|^2 - 2 x.y + |y|^2, whose absolute error is ~eps |x|^2: enough to pick the winner (up to ties
// inside that noise), not to report a tiny distance -- a duplicated cell would come out as ~1e-7 |x| instead of 0, and the
// reference replaces exactly the non-positive distances (validation.py:528-592).  The reported value is therefore
// recomputed from the winner's coordinates: sum (x_k - y_k)^2, relative error ~eps.
__device__ __forceinline__ double nn_direct_distance(const double* __restrict__ x, int64_t i, const double* __restrict__ y,
                                                     int64_t j, int d) {
  if (j < 0) return INFINITY;
  double s = 0.0;
  for (int k = 0; k < d; ++k) {
    const double t = x[i * d + k] - y[j * d + k];
    s = fma(t, t, s);
  }
  return sqrt(s);
}

// Exact Euclidean nearest-neighbour distance of every row of x among the rows of y, skipping the
// pair (i, i + self_offset).  Replaces the approximate pynndescent search of the reference
// (mellon/parameters.py:352-433) -- same tile structure as the covariance kernel; the running
// minimum of the squared distance stays in registers across all centre tiles.
__global__ __launch_bounds__(256) void k_nn_distances(const double* __restrict__ x, int64_t n,
                                                      const double* __restrict__ y, int64_t m, int d,
                                                      const double* __restrict__ xx,
                                                      const double* __restrict__ yy, int64_t self_offset,
                                                      const int64_t* __restrict__ excl, double* __restrict__ out) {
  __shared__ double xs[DK][TM + PADT];
  __shared__ double ys[DK][TN + PADT];
  __shared__ double red[TM][17];
  __shared__ int64_t redj[TM][17];
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * TM;
  double best[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
  int64_t bj[4] = {-1, -1, -1, -1};
  double xr[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int64_t r = row0 + ty * 4 + i;
    xr[i] = (r < n) ? xx[r] : 0.0;
  }
  for (int64_t col0 = 0; col0 < m; col0 += TN) {
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    for (int k0 = 0; k0 < d; k0 += DK) {
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        int idx = tid + 256 * q;
        int r = idx >> 4, k = idx & 15;
        double vx = 0.0, vy = 0.0;
        if (k0 + k < d) {
          if (row0 + r < n) vx = x[(row0 + r) * (int64_t)d + k0 + k];
          if (col0 + r < m) vy = y[(col0 + r) * (int64_t)d + k0 + k];
        }
        xs[k][r] = vx;
        ys[k][r] = vy;
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < DK; ++k) {
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
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t c = col0 + tx * 4 + j;
      const double yj = (c < m) ? yy[c] : 0.0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t r = row0 + ty * 4 + i;
        const double sq = xr[i] - 2.0 * acc[i][j] + yj;
        const int64_t skip = (excl && r < n) ? excl[r] : r + self_offset;
        if (c < m && c != skip && sq < best[i]) { best[i] = sq; bj[i] = c; }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) { red[ty * 4 + i][tx] = best[i]; redj[ty * 4 + i][tx] = bj[i]; }
  __syncthreads();
  if (tid < TM) {
    double s = INFINITY;
    int64_t j = -1;
#pragma unroll
    for (int t = 0; t < 16; ++t)
      if (red[tid][t] < s) { s = red[tid][t]; j = redj[tid][t]; }
    int64_t r = row0 + tid;
    if (r < n) out[r] = nn_direct_distance(x, r, y, j, d);
  }
}

// Exact 1-NN on the matrix cores (d <= 64): a workgroup of 8 waves owns 128 query rows, every wave keeps the
// MFMA A operands of its 16 rows in registers for the whole pass and walks all tiles of 64 candidate rows,
// which are staged through LDS once per workgroup (double-buffered, coalesced in, [row][k] with a
// 68-double row stride out) and shared by the 8 waves.  Only xx - 2 x.y + yy and a running minimum per
// element: the pass is bound by the fp64 matrix pipe (2 n m d flops).

__global__ __launch_bounds__(512) void k_nn_distances_mfma(const double* __restrict__ x, int64_t n,
                                                           const double* __restrict__ y, int64_t m, int d,
                                                           const double* __restrict__ xx,
                                                           const double* __restrict__ yy, int64_t self_offset,
                                                           const int64_t* __restrict__ excl, double* __restrict__ out) {
  __shared__ double ys[2][TN * NNS];
  __shared__ double yn[2][TN];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * 128 + wave * 16;
  const int ksteps = (d + 3) / 4;
  // A operands of this wave's 16 rows: a[ks] = x[row0 + li][4 ks + lk]
  double a[16];
  {
    const int64_t ar = (row0 + li < n) ? row0 + li : n - 1;
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
      const int k = 4 * ks + lk;
      a[ks] = (ks < ksteps && k < d) ? x[ar * d + k] : 0.0;
    }
  }
  double xr[4], best[4];
  int bt[4];            // the winner so far as a 16-column group: column = 16 bt + li (bt < 2^31: m < 2^35)
  int64_t ex[4];        // the candidate that does not count for each of this lane's rows
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t row = row0 + lk + 4 * r;
    xr[r] = (row < n) ? xx[row] : 0.0;
    ex[r] = (excl && row < n) ? excl[row] : row + self_offset;
    best[r] = INFINITY;
    bt[r] = -1;
  }
  for (int e = tid; e < 2 * TN * NNS; e += 512) (&ys[0][0])[e] = 0.0;   // zero incl. the k padding
  __syncthreads();
  auto stage = [&](int buf, int64_t col0) {
    const int cnt = TN * d;
    for (int e = tid; e < cnt; e += 512) {
      const int r = e / d, k = e - r * d;
      ys[buf][r * NNS + k] = (col0 + r < m) ? y[(col0 + r) * d + k] : 0.0;
    }
    if (tid < TN) yn[buf][tid] = (col0 + tid < m) ? yy[col0 + tid] : 0.0;
  };
  stage(0, 0);
  __syncthreads();
  int buf = 0;
  for (int64_t col0 = 0; col0 < m; col0 += TN, buf ^= 1) {
    if (col0 + TN < m) stage(buf ^ 1, col0 + TN);
    v4d_t acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = v4d_t{0.0, 0.0, 0.0, 0.0};
    const double* yb = &ys[buf][li * NNS + lk];
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
      if (ks < ksteps) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
          acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], yb[16 * t * NNS + 4 * ks], acc[t], 0, 0, 0);
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int64_t c = col0 + 16 * t + li;
      const double yc = yn[buf][16 * t + li];
      const int grp = (int)(col0 >> 4) + t;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double sq = xr[r] - 2.0 * acc[t][r] + yc;
        if (c < m && c != ex[r] && sq < best[r]) { best[r] = sq; bt[r] = grp; }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double s_ = best[r];
    int64_t j_ = bt[r] < 0 ? -1 : 16 * (int64_t)bt[r] + li;
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) {
      const double so = __shfl_xor(s_, off, 64);
      const int64_t jo = __shfl_xor(j_, off, 64);
      if (so < s_ || (so == s_ && jo >= 0 && (j_ < 0 || jo < j_))) { s_ = so; j_ = jo; }
    }
    const int64_t row = row0 + lk + 4 * r;
    if (li == 0 && row < n) out[row] = nn_direct_distance(x, row, y, j_, d);
  }
}

__global__ void k_row_sqnorms_all(const double* __restrict__ x, int64_t n, int d, double* __restrict__ xx) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int k = 0; k < d; ++k) {
    double v = x[i * (int64_t)d + k];
    s = fma(v, v, s);
  }
  xx[i] = s;
}

// diag_i = cov(x_i, x_i) (reference base_cov.py:71-93): the whole program with xy = xx = yy per leaf.
__global__ void k_cov_diag(DevCov cov, const double* __restrict__ x, int64_t n, int d, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  int sp = 0;
  for (int t = 0; t < cov.n_toks; ++t) {
    const int op = cov.tok_op[t];
    if (op == MLN_OP_LEAF || op == MLN_OP_CONST) {
      double v;
      if (op == MLN_OP_CONST) {
        v = cov.tok_val[t];
      } else {
        const DevLeaf lf = cov.leaves[cov.tok_leaf[t]];
        double xx = 0.0;
        for (int k = 0; k < lf.ndims; ++k) {
          const double q = x[i * (int64_t)d + cov.dims[lf.dims_off + k]];
          xx = fma(q, q, xx);
        }
        v = leaf_value(lf, xx, xx, xx);
      }
      if (sp > 0) { s2 = s1; s1 = s0; }
      s0 = v;
      ++sp;
    } else {
      const double l = s1, r = s0;
      s0 = (op == MLN_OP_ADD) ? (l + r) : (op == MLN_OP_MUL) ? (l * r) : pow(l, r);
      s1 = s2;
      --sp;
    }
  }
  out[i] = s0;
}

// out_i = base_i + sign * sum_j T_ij^2 [* scale_j^2]
__global__ void k_row_sumsq(const double* __restrict__ T, int64_t ld, int64_t rows, int64_t cols,
                            const double* __restrict__ base, double sign, double* __restrict__ out) {
  const int64_t i = blockIdx.x;
  if (i >= rows) return;
  __shared__ double red[256];
  double s = 0.0;
  for (int64_t j = threadIdx.x; j < cols; j += 256) { const double v = T[i * ld + j]; s = fma(v, v, s); }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[i] = (base ? base[i] : 0.0) + sign * red[0];
}

}  // namespace

// xx[leaf][i] = |x_i|dims|^2: the pass every covariance-tile launcher starts with (here, cov_predict_deriv.hip, cov_block_deriv.hip)
int launch_leaf_sqnorms(mln_ctx* ctx, const DevCov& cov, const double* x, int64_t n, int d, double* xx) {
  if (n == 0) return MLN_OK;
  hipLaunchKernelGGL(k_row_sqnorms, dim3((unsigned)((n + 31) / 32)), dim3(256), 0, ctx->stream, cov, x, n, d, xx);
  MLN_HIP(ctx, hipGetLastError());
  return MLN_OK;
}

// The persistent-row kernels (rows_pipeline.h: cov_rows_impl.h, predict_rows_impl.h; kernel_rows_prod_impl.h) stage centre tiles without
// bounds checks: they are handed a COPY of the centres followed by ROWS_PAD zero rows (and norms / weights padded alike).
constexpr int64_t ROWS_PAD = 3 * 64;   // (a predict kernel requests tile t + 2 up to t = ceil(m / 64) - 1)
static int pad_rows(mln_ctx* ctx, const double* src, int64_t rows, int64_t cols, double* dst) {
  MLN_HIP(ctx, hipMemcpyAsync(dst, src, sizeof(double) * (size_t)(rows * cols), hipMemcpyDeviceToDevice, ctx->stream));
  MLN_HIP(ctx, hipMemsetAsync(dst + rows * cols, 0, sizeof(double) * (size_t)(ROWS_PAD * cols), ctx->stream));
  return MLN_OK;
}

int launch_kernel_matrix(mln_ctx* ctx, const DevCov& cov, const double* x, int64_t n, const double* y,
                         int64_t m, int d, double* out, int64_t ldo, double add_diag, float* out32, int q32) {
  if (n == 0 || m == 0) return MLN_OK;
  double* norms = nullptr;
  const int64_t mp = m + ROWS_PAD;
  MLN_TRY(mln_scratch(ctx, sizeof(double) * ((size_t)cov.n_leaves * (size_t)(n + mp) + (size_t)(mp * d)), (void**)&norms));
  double* xx = norms;
  double* yy = norms + (int64_t)cov.n_leaves * n;
  double* ypad = yy + (int64_t)cov.n_leaves * mp;
  MLN_TRY(launch_leaf_sqnorms(ctx, cov, x, n, d, xx));
  MLN_TRY(launch_leaf_sqnorms(ctx, cov, y, m, d, yy));
  const int64_t tiles_n = (ldo + TN - 1) / TN, tiles_m = (n + TM - 1) / TM;   // covers the pad columns too
  const int64_t nblk = tiles_n * tiles_m;
  if (nblk > 0x7fffffffLL) { mln_set_error(ctx, "kernel matrix too large for one launch"); return MLN_ERR_UNSUPPORTED; }
  const bool single = (cov.n_toks == 1);
  bool contiguous = single && cov.leaves[0].ndims == d;
  if (contiguous)
    for (int k = 0; k < d; ++k) contiguous = contiguous && cov.dims[cov.leaves[0].dims_off + k] == k;
  static const bool no_rows_env = mln_experiment("MELLON_AMD_KM_NO_ROWS") != nullptr;
  // (the persistent-row kernels read the centres WITHOUT bounds checks up to tile ceil(ldo / 64) + 1: the zero rows pad_rows
  //  appends cover that only while the output's leading dimension stays within 64 columns of m -- every caller passes
  //  ldo = m or pad16(m); anything wider takes the tiled kernels)
  const bool no_rows = no_rows_env || ldo > m + 64;
  if (contiguous && !no_rows && d <= 64 && n >= 4096 && m >= 256 && cov.leaves[0].kind != MLN_K_LINEAR &&
      cov.leaves[0].kind != MLN_K_DISTANCE && cov.leaves[0].kind != MLN_K_RATQUAD && (!out32 || q32)) {
    MLN_TRY(pad_rows(ctx, y, m, d, ypad));
    MLN_HIP(ctx, hipMemsetAsync(yy + m, 0, sizeof(double) * (size_t)ROWS_PAD, ctx->stream));   // norms of the pad rows
    MLN_TRY(launch_kernel_matrix_rows_q(ctx, cov, x, n, ypad, m, d, xx, yy, out, ldo, add_diag, out32, q32));
  } else if (!no_rows && n >= 4096 && m >= 256 && (!out32 || q32) && predict_rows_prod_eligible(cov, d)) {
    // the time-sensitive product kernel: state leaf x time leaf, both in the persistent-row kernel (leaf 0's norms come
    // first; leaf 1's, which it does not use, are overwritten by the zero padding)
    MLN_TRY(pad_rows(ctx, y, m, d, ypad));
    MLN_HIP(ctx, hipMemsetAsync(yy + m, 0, sizeof(double) * (size_t)ROWS_PAD, ctx->stream));
    MLN_TRY(launch_kernel_matrix_rows_prod(ctx, cov, x, n, ypad, m, d, xx, yy, out, ldo, add_diag, out32, q32));
  } else if (contiguous && n * m >= 4096)
    hipLaunchKernelGGL(k_kernel_matrix_mfma, dim3((unsigned)nblk), dim3(256), 0, ctx->stream, cov, x, n, y, m, d,
                       xx, yy, out, ldo, add_diag, tiles_n, out32, q32);
  else if (single)
    hipLaunchKernelGGL(k_kernel_matrix<true>, dim3((unsigned)nblk), dim3(256), 0, ctx->stream, cov, x, n, y, m, d,
                       xx, yy, out, ldo, add_diag, tiles_n, out32, q32);
  else
    hipLaunchKernelGGL(k_kernel_matrix<false>, dim3((unsigned)nblk), dim3(256), 0, ctx->stream, cov, x, n, y, m, d,
                       xx, yy, out, ldo, add_diag, tiles_n, out32, q32);
  MLN_HIP(ctx, hipGetLastError());
  return MLN_OK;
}

int launch_predict_mean1(mln_ctx* ctx, const DevCov& cov, const double* x, int64_t n, const double* y,
                         int64_t m, int d, const double* w, double mu, double* out) {
  if (n == 0) return MLN_OK;
  double* norms = nullptr;
  const int64_t mp = m + ROWS_PAD;
  MLN_TRY(mln_scratch(ctx, sizeof(double) * ((size_t)cov.n_leaves * (size_t)(n + mp) + (size_t)(mp * (d + 1))), (void**)&norms));
  double* xx = norms;
  double* yy = norms + (int64_t)cov.n_leaves * n;
  double* ypad = yy + (int64_t)cov.n_leaves * mp;
  double* wpad = ypad + mp * d;
  MLN_TRY(launch_leaf_sqnorms(ctx, cov, x, n, d, xx));
  MLN_TRY(launch_leaf_sqnorms(ctx, cov, y, m, d, yy));
  const int64_t nblk = (n + TM - 1) / TM;
  const bool single = (cov.n_toks == 1);
  bool contiguous = single && cov.leaves[0].ndims == d;
  if (contiguous)
    for (int k = 0; k < d; ++k) contiguous = contiguous && cov.dims[cov.leaves[0].dims_off + k] == k;
  if (contiguous && d <= 64 && n >= 4096 && m >= 256 && cov.leaves[0].kind != MLN_K_LINEAR &&
      cov.leaves[0].kind != MLN_K_DISTANCE) {
    MLN_TRY(pad_rows(ctx, y, m, d, ypad));
    MLN_TRY(pad_rows(ctx, w, m, 1, wpad));
    MLN_HIP(ctx, hipMemsetAsync(yy + m, 0, sizeof(double) * (size_t)ROWS_PAD, ctx->stream));
    MLN_TRY(launch_predict_mean_rows(ctx, cov, x, n, ypad, m, d, xx, yy, wpad, mu, out));
  } else if (n >= 4096 && m >= 256 && predict_rows_prod_eligible(cov, d)) {
    MLN_TRY(pad_rows(ctx, y, m, d, ypad));
    MLN_TRY(pad_rows(ctx, w, m, 1, wpad));
    MLN_HIP(ctx, hipMemsetAsync(yy + m, 0, sizeof(double) * (size_t)ROWS_PAD, ctx->stream));   // (leaf 0's norms come first)
    MLN_TRY(launch_predict_mean_rows_prod(ctx, cov, x, n, ypad, m, d, xx, yy, wpad, mu, out));
  } else if (contiguous && n * m >= 4096)
    hipLaunchKernelGGL(k_predict_mean_mfma, dim3((unsigned)nblk), dim3(256), 0, ctx->stream, cov, x, n, y, m, d,
                       xx, yy, w, mu, out);
  else if (single)
    hipLaunchKernelGGL(k_predict_mean1<true>, dim3((unsigned)nblk), dim3(256), 0, ctx->stream, cov, x, n, y, m, d,
                       xx, yy, w, mu, out);
  else
    hipLaunchKernelGGL(k_predict_mean1<false>, dim3((unsigned)nblk), dim3(256), 0, ctx->stream, cov, x, n, y, m, d,
                       xx, yy, w, mu, out);
  MLN_HIP(ctx, hipGetLastError());
  return MLN_OK;
}

int launch_nn_distances_exact(mln_ctx* ctx, const double* x, int64_t n, const double* y, int64_t m, int d,
                              int64_t self_offset, const int64_t* excl, double* out) {
  if (n == 0) return MLN_OK;
  DevBuf<double> norms;
  MLN_TRY(norms.alloc(ctx, (size_t)(n + m), "norms"));
  double* xx = norms;
  double* yy = norms + n;
  hipLaunchKernelGGL(k_row_sqnorms_all, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, x, n, d, xx);
  hipLaunchKernelGGL(k_row_sqnorms_all, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, y, m, d, yy);
  if (d <= 64 && n * m >= 4096)
    hipLaunchKernelGGL(k_nn_distances_mfma, dim3((unsigned)((n + 127) / 128)), dim3(512), 0, ctx->stream, x, n, y, m, d,
                       xx, yy, self_offset, excl, out);
  else
    hipLaunchKernelGGL(k_nn_distances, dim3((unsigned)((n + TM - 1) / TM)), dim3(256), 0, ctx->stream, x, n, y, m, d,
                       xx, yy, self_offset, excl, out);
  hipError_t e = hipGetLastError();
  (void)hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) return mln_hip_fail(ctx, e, "nn_distances", __FILE__, __LINE__);
  return MLN_OK;
}

// Exact nearest-neighbour distances.  Large searches (d <= 64) go through the fp16 pre-filter with fp64 certification
// (rowmin_f16.hip): same result, a fraction of the time.  MELLON_AMD_NN_PREFILTER=0 forces the plain fp64 search.
int launch_nn_distances(mln_ctx* ctx, const double* x, int64_t n, const double* y, int64_t m, int d,
                        int64_t self_offset, double* out) {
  if (n == 0) return MLN_OK;
  const char* e_on = std::getenv("MELLON_AMD_NN_PREFILTER");          // read per call: the tests flip it
  const char* e_min = std::getenv("MELLON_AMD_NN_PREFILTER_MIN");
  const bool prefilter = !(e_on && std::atoi(e_on) == 0);
  const int64_t min_pairs = e_min ? std::atoll(e_min) : ((int64_t)1 << 26);
  // what this call did, for mln_diag_nn_last: the pre-filter routes fill it in themselves (2, 3, 4 and their open rows)
  ctx->nn_last[0] = (d <= 64 && n * m >= 4096) ? 1.0 : 0.0;
  ctx->nn_last[1] = ctx->nn_last[2] = ctx->nn_last[3] = 0.0;
  if (prefilter && d <= 64 && m >= 2 && n * m >= min_pairs && m < 2147483647LL)
    return nn_distances_prefiltered(ctx, x, n, y, m, d, self_offset, out, nullptr);
  if (prefilter && d <= ROWMIN_WIDE_MAX_D && m >= 2 && n * m >= min_pairs && m < 2147483647LL && n < 2147483647LL)      // (65 <= d: rowmin_wide.hip)
    return nn_distances_wide(ctx, x, n, y, m, d, self_offset, out);
  return launch_nn_distances_exact(ctx, x, n, y, m, d, self_offset, nullptr, out);
}

int launch_cov_diag(mln_ctx* ctx, const DevCov& cov, const double* x, int64_t n, int d, double* out) {
  if (n == 0) return MLN_OK;
  hipLaunchKernelGGL(k_cov_diag, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, cov, x, n, d, out);
  MLN_HIP(ctx, hipGetLastError());
  return MLN_OK;
}

int launch_row_sumsq(mln_ctx* ctx, const double* T, int64_t ld, int64_t rows, int64_t cols, const double* base,
                     double sign, double* out) {
  if (rows == 0) return MLN_OK;
  hipLaunchKernelGGL(k_row_sumsq, dim3((unsigned)rows), dim3(256), 0, ctx->stream, T, ld, rows, cols, base, sign, out);
  MLN_HIP(ctx, hipGetLastError());
  return MLN_OK;
}

