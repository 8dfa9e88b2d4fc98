// mln_dim_objective at S points in one call (the Monte-Carlo step of DimensionalityEstimator(optimizer="advi"); the
// reference vmaps its loss over nsamples = 40 draws).  Per sample the arithmetic is mln_dim_objective's (dimensionality.hip,
// dim_process), with z = (z0, z1) the two latent functions of the sample:
//   f0 = L z0,  f1 = L z1,  D = exp(mu_dim + f0),  pred_j = mu_dens + f1 + D ell_j - lnGamma(D / 2 + 1),
//   loss = 1/2 |z|^2 + log 2 pi - sum_i sum_j [pred_ij j - exp(pred_ij) - lnGamma(j)],
//   grad = z + [L^T c0 ; L^T c1],  c1_i = -sum_j (j - e_ij),  c0_i = -D_i sum_j (j - e_ij)(ell_ij - psi(D_i / 2 + 1) / 2).
//
// The structure is objective_batch.hip's with two columns per sample: the S points share the n x m buffer, which is
// read twice per chunk of samples, not once per sample.
//
//   k_dim_batch_forward  F = B W  (n x m times m x 2 SP, SP = the chunk's samples padded to a multiple of 16; columns
//                        [0, SP) hold the z0 of the samples, [SP, 2 SP) their z1) on v_mfma_f64_16x16x4_f64, the tile
//                        and the main loop of k_batch_forward.  With the C layout col = lane & 15, accumulator tiles j and
//                        NT + j of a lane hold f0 and f1 of the same (row, sample): the epilogue needs no exchange.  Per
//                        (row, sample) it computes D, lnGamma / psi of D / 2 + 1 (gamma_fns, dim_gamma.h) and the k Poisson
//                        terms over ell[row][0 .. k), and stores c0 into column s and c1 into column SP + s of an
//                        n x 2 SP matrix.  F is never written.  The tile's likelihood sums: lanes, then waves, fixed order.
//   k_batch_backward     G = B^T [C0 | C1]  (m x 2 SP): objective_batch.h's kernel with 2 NT column tiles, then k_batch_sum.
//
// The backward kernel holds at most four column tiles, so a chunk is 32 samples (2 NT <= 4): S = 40 reads the buffer
// four times per call.  Every sum has a fixed order: two calls give identical bits.  Every handle is batched as in
// objective_batch.hip (implicit: W = Lp^-T [Z0 | Z1] before, Lp^-1 G after, 2 SP right-hand sides); the 5120-column limit of
// the single pass is inherited through mln_fit_set_dim_likelihood.
#include "api_internal.h"
#include "dim_gamma.h"
#include "objective_batch.h"

namespace {

constexpr int DIM_S_CHUNK = 32;   // samples per launch: two accumulator columns per sample, four per wave

// NT: sample tiles of 16 (the product has 2 NT column tiles)
template <int NT>
__global__ __launch_bounds__(256, 2) void k_dim_batch_forward(const double* __restrict__ B, int64_t ldb, int64_t n, int64_t kdim,
                                                             const double* __restrict__ W, const double* __restrict__ ell,
                                                             int k, int S, double mu_dim, double mu_dens,
                                                             double* __restrict__ C, double* __restrict__ part_loss) {
  constexpr int CT = 2 * NT, SP = 16 * NT, SP2 = 2 * SP, WLD = SkinnyLd<CT>::v;
  __shared__ __attribute__((aligned(16))) double As[BT][A_LD];
  __shared__ double Ws[BK][WLD];
  __shared__ double lred[4][SP];
  __shared__ double lgj[64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lk = lane >> 4, li = lane & 15;
  const int64_t r0 = (int64_t)blockIdx.x * BT;
  if (t < 64) lgj[t] = lgamma((double)(t + 1));   // lnGamma(j), j = 1 .. 64 (read after the main loop's barriers)

  v4d acc[4][CT];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < CT; ++j) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};

  d2 ra[8];
  double rw[CT];
  // buffer tile: 256 rows x 16 k; eight consecutive lanes read one row's 128 bytes (kdim = ldb is a multiple of 16)
  auto load_tiles = [&](int64_t k0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int idx = t + 256 * q;
      const int64_t gr = r0 + (idx >> 3);
      ra[q] = (gr < n) ? __builtin_nontemporal_load(reinterpret_cast<const d2*>(B + gr * ldb + k0) + (idx & 7)) : (d2){0.0, 0.0};
    }
#pragma unroll
    for (int q = 0; q < CT; ++q) rw[q] = W[k0 * SP2 + t + 256 * q];   // W has kdim rows (zero beyond m): 16 x 2 SP contiguous
  };
  load_tiles(0);
  for (int64_t k0 = 0; k0 < kdim; k0 += BK) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int idx = t + 256 * q;
      *reinterpret_cast<d2*>(&As[idx >> 3][2 * (idx & 7)]) = ra[q];
    }
#pragma unroll
    for (int q = 0; q < CT; ++q) {
      const int idx = t + 256 * q;
      Ws[idx / SP2][idx % SP2] = rw[q];
    }
    __syncthreads();
    if (k0 + BK < kdim) load_tiles(k0 + BK);
#pragma unroll
    for (int kk = 0; kk < BK; kk += 4) {
      double a[4], b[CT];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = As[wave * 64 + i * 16 + li][kk + lk];
#pragma unroll
      for (int j = 0; j < CT; ++j) b[j] = Ws[kk + lk][j * 16 + li];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < CT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }
  // C/D layout of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * reg.  Tiles j and NT + j: f0 and f1 of
  // sample 16 j + li.  Rows past n read row n - 1 (n >= 1) and store nothing; padding samples (>= S) store zeros.
  double ls[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) ls[j] = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = r0 + wave * 64 + i * 16 + lk + 4 * r;
      const bool ok = row < n;
      const double* er = ell + (ok ? row : (n - 1)) * k;
      double D[NT], fd[NT], lg[NT], ps[NT], sa[NT], sas[NT], sl[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        D[j] = exp(mu_dim + acc[i][j][r]);                  // inference.py:160-162: dims = exp(mu_dim + L z0)
        fd[j] = mu_dens + acc[i][NT + j][r];
        double tp;
        gamma_fns<false>(0.5 * D[j] + 1.0, lg[j], ps[j], tp);
        sa[j] = sas[j] = sl[j] = 0.0;
      }
      // the Poisson terms (inference.py:112-120): pred = log_dens + D ell - lgamma(D / 2 + 1), neighbour counts 1 .. k
      for (int q = 0; q < k; ++q) {
        const double e_l = er[q], cnt = (double)(q + 1), lgq = lgj[q];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const double pred = fd[j] + D[j] * e_l - lg[j];
          const double e = exp(pred);
          const double av = cnt - e;
          sa[j] += av;
          sas[j] = fma(av, e_l - 0.5 * ps[j], sas[j]);
          sl[j] += fma(pred, cnt, -e) - lgq;
        }
      }
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const bool live = 16 * j + li < S;
        if (ok) {
          if (live) ls[j] += sl[j];
          C[row * SP2 + j * 16 + li] = live ? -D[j] * sas[j] : 0.0;          // d loss / d (L z0)_row
          C[row * SP2 + SP + j * 16 + li] = live ? -sa[j] : 0.0;             // d loss / d log_dens_row
        }
      }
    }
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    ls[j] += __shfl_xor(ls[j], 16, 64);
    ls[j] += __shfl_xor(ls[j], 32, 64);
    if (lk == 0) lred[wave][j * 16 + li] = ls[j];
  }
  __syncthreads();
  if (t < SP) part_loss[(int64_t)blockIdx.x * SP + t] = -((lred[0][t] + lred[1][t]) + (lred[2][t] + lred[3][t]));
}

// W[j][c] (ldl x 2 SP, zero beyond m rows / S samples): column c = s holds z0 of sample s, column SP + s its z1
__global__ __launch_bounds__(256) void k_dim_batch_z_to_w(const double* __restrict__ Z, int S, int64_t m, int SP, int64_t rows,
                                                          double* __restrict__ W) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * 2 * SP) return;
  const int64_t j = i / (2 * SP);
  const int c = (int)(i % (2 * SP));
  const int s = c % SP, lat = c / SP;
  W[i] = (j < m && s < S) ? Z[((int64_t)s * 2 + lat) * m + j] : 0.0;
}

// prior terms, added once per sample, with the reference's K = 2 latent functions in the constant (mln_dim_objective), and
// the gradient back in sample-major order:
//   loss[s] = lik[s] + 1/2 |z_s|^2 (2 m entries) + log 2 pi,  grad[s][0][j] = G[j][s] + z,  grad[s][1][j] = G[j][SP + s] + z
__global__ __launch_bounds__(256) void k_dim_batch_finish(const double* __restrict__ Z, int64_t m, int SP,
                                                          const double* __restrict__ lik, const double* __restrict__ G,
                                                          double* __restrict__ loss, double* __restrict__ grad) {
  __shared__ double red[256];
  const int s = blockIdx.x, t = threadIdx.x;
  const double* z = Z + (int64_t)s * 2 * m;
  double* g = grad + (int64_t)s * 2 * m;
  double zz = 0.0;
  for (int64_t j = t; j < m; j += 256) {
    const double v0 = z[j], v1 = z[m + j];
    zz = fma(v0, v0, zz);
    zz = fma(v1, v1, zz);
    g[j] = G[j * 2 * SP + s] + v0;
    g[m + j] = G[j * 2 * SP + SP + s] + v1;
  }
  red[t] = zz;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (t < off) red[t] += red[t + off];
    __syncthreads();
  }
  if (t == 0) {
    const double lv = lik[s] + 0.5 * red[0] + 1.8378770664093453;   // log(2 pi)
    loss[s] = isfinite(lv) ? lv : __builtin_inf();                  // as mln_dim_objective: a non-finite point reads as +inf
  }
}

template <int NT>
int launch_dim_batch(mln_fit* f, const double* W, int S, double* C, double* part_loss, int64_t n_tiles, double* part,
                     int n_ranges, int64_t rows_per_range) {
  mln_ctx* ctx = f->ctx;
  hipLaunchKernelGGL((k_dim_batch_forward<NT>), dim3((unsigned)n_tiles), dim3(256), 0, ctx->stream, f->L, f->ldl, f->n, f->ldl,
                     W, f->dim_ell, f->dim_k, S, f->mu_dim, f->mu_dens, C, part_loss);
  MLN_HIP(ctx, hipGetLastError());
  const unsigned col_blocks = (unsigned)((f->ldl + BT - 1) / BT);
  hipLaunchKernelGGL((k_batch_backward<2 * NT>), dim3(col_blocks, (unsigned)n_ranges), dim3(256), 0, ctx->stream, f->L, f->ldl,
                     f->n, rows_per_range, C, part);
  MLN_HIP(ctx, hipGetLastError());
  return MLN_OK;
}

}  // namespace

extern "C" int mln_dim_objective_batch(mln_fit* f, const double* Z, int32_t S, double* loss, double* grad) {
  if (!f || !Z || !loss || !grad || S < 1) return MLN_ERR_ARG;
  mln_ctx* ctx = f->ctx;
  if (!f->dim_ell) { mln_set_error(ctx, "mln_fit_set_dim_likelihood has not been called"); return MLN_ERR_ARG; }
  MLN_HIP(ctx, hipSetDevice(ctx->device));
  MLN_TRY(fit_ensure_lp(f));
  const int64_t m = f->m, ldl = f->ldl, n = f->n;
  const int sp_max = 16 * (int)((std::min<int64_t>(S, DIM_S_CHUNK) + 15) / 16);
  // row ranges of the backward kernel: about four workgroups per CU, at least 256 cells each (as mln_objective_batch)
  const int64_t col_blocks = (ldl + BT - 1) / BT;
  const int64_t n_cu = ctx->n_cu > 0 ? ctx->n_cu : 256;
  int64_t n_ranges = std::max<int64_t>(1, (4 * n_cu) / col_blocks);
  n_ranges = std::min<int64_t>(n_ranges, std::max<int64_t>(1, (n + 255) / 256));
  const int64_t rows_per_range = std::max<int64_t>(16, (((n + n_ranges - 1) / n_ranges) + 15) / 16 * 16);
  const int64_t n_tiles = (n + BT - 1) / BT;
  // one block: Z chunk | W | [lik ; G] (all-reduced together) | [C0 | C1] | likelihood partials | gradient partials | loss, grad out
  const size_t c_z = (size_t)sp_max * 2 * m, c_w = (size_t)ldl * 2 * sp_max, c_lg = (size_t)sp_max * (1 + 2 * ldl),
               c_c = (size_t)std::max<int64_t>(n, 1) * 2 * sp_max, c_pl = (size_t)std::max<int64_t>(n_tiles, 1) * sp_max,
               c_part = (size_t)n_ranges * ldl * 2 * sp_max, c_out = (size_t)sp_max * (1 + 2 * m);
  auto even = [](size_t c) { return (c + 1) & ~(size_t)1; };
  DevBuf<double> sc;
  MLN_TRY(sc.alloc(ctx, even(c_z) + even(c_w) + even(c_lg) + even(c_c) + even(c_pl) + even(c_part) + even(c_out),
                   "batched dimensionality objective workspace"));
  double* d_Z = sc;
  double* d_W = d_Z + even(c_z);
  double* d_lg = d_W + even(c_w);
  double* d_C = d_lg + even(c_lg);
  double* d_pl = d_C + even(c_c);
  double* d_part = d_pl + even(c_pl);
  double* d_out = d_part + even(c_part);

  for (int32_t s0 = 0; s0 < S; s0 += DIM_S_CHUNK) {
    const int Sc = std::min<int32_t>(DIM_S_CHUNK, S - s0);
    const int NT = (Sc + 15) / 16, SP = 16 * NT, SP2 = 2 * SP;
    double* d_lik = d_lg;
    double* d_G = d_lg + SP;
    MLN_HIP(ctx, hipMemcpyAsync(d_Z, Z + (int64_t)s0 * 2 * m, sizeof(double) * (size_t)Sc * 2 * m, hipMemcpyDefault, ctx->stream));
    hipLaunchKernelGGL(k_dim_batch_z_to_w, dim3((unsigned)((ldl * SP2 + 255) / 256)), dim3(256), 0, ctx->stream, d_Z, Sc, m, SP, ldl, d_W);
    MLN_HIP(ctx, hipGetLastError());
    if (f->kspace) MLN_TRY(triinv_solve_left_T(ctx, f->tri, d_W, SP2, SP2));         // W = Lp^-T [Z0 | Z1]
    if (n > 0) {
      int rc = MLN_OK;
      if (NT == 1) rc = launch_dim_batch<1>(f, d_W, Sc, d_C, d_pl, n_tiles, d_part, (int)n_ranges, rows_per_range);
      else rc = launch_dim_batch<2>(f, d_W, Sc, d_C, d_pl, n_tiles, d_part, (int)n_ranges, rows_per_range);
      MLN_TRY(rc);
      hipLaunchKernelGGL(k_batch_loss_sum, dim3((unsigned)SP), dim3(256), 0, ctx->stream, d_pl, n_tiles, SP, d_lik);
      MLN_HIP(ctx, hipGetLastError());
      hipLaunchKernelGGL(k_batch_sum, dim3((unsigned)((ldl * SP2 + 255) / 256)), dim3(256), 0, ctx->stream, d_part, (int)n_ranges, ldl * SP2, d_G,
                         ldl * SP2);
      MLN_HIP(ctx, hipGetLastError());
    } else {                                                                        // a rank without cells
      MLN_HIP(ctx, hipMemsetAsync(d_lg, 0, sizeof(double) * (size_t)SP * (1 + 2 * ldl), ctx->stream));
    }
    MLN_TRY(dev_allreduce(ctx, d_lg, (int64_t)SP * (1 + 2 * ldl)));
    if (f->kspace) MLN_TRY(triinv_solve_left(ctx, f->tri, d_G, SP2, SP2));           // L^T v = Lp^-1 (K^T v)
    double* o_loss = d_out;
    double* o_grad = d_out + SP;
    hipLaunchKernelGGL(k_dim_batch_finish, dim3((unsigned)Sc), dim3(256), 0, ctx->stream, d_Z, m, SP, d_lik, d_G, o_loss, o_grad);
    MLN_HIP(ctx, hipGetLastError());
    MLN_HIP(ctx, hipMemcpyAsync(loss + s0, o_loss, sizeof(double) * (size_t)Sc, hipMemcpyDefault, ctx->stream));
    MLN_HIP(ctx, hipMemcpyAsync(grad + (int64_t)s0 * 2 * m, o_grad, sizeof(double) * (size_t)Sc * 2 * m, hipMemcpyDefault, ctx->stream));
    MLN_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return MLN_OK;
}
