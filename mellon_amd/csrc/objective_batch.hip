// mln_objective at S points in one call (the Monte-Carlo step of optimizer="advi", mellon/inference.py:768-876: the
// reference vmaps its loss over nsamples = 40 draws).  Per sample the arithmetic is mln_objective's:
//   f = L z + mu,  a = exp(f + V),  loss = 1/2 |z|^2 + (m/2) log 2 pi - sum_i (f_i + Vdr_i - a_i),  grad = z + L^T (a - 1).
//
// The S points share the n x m buffer, so the work is two skinny fp64 matrix products around the likelihood.  The m x S
// gradient block (1.9 MB at m = 5000, S = 48) fits neither the LDS nor the registers of a CU, so the single-read fusion of
// k_objective is not available; the buffer is read twice, not S times:
//
//   k_batch_forward   F = B W  (n x m times m x SP, SP = S padded to a multiple of 16) on v_mfma_f64_16x16x4_f64.
//                     One workgroup owns a 256-row x SP tile (4 waves x 64 rows x SP: 4 x SP/16 accumulators each), so no
//                     matrix instruction is spent on columns beyond SP.  Epilogue: + mu, a = exp(f + V), the SP likelihood
//                     sums of the tile (lanes, then waves, fixed order), and a - 1 stored (n x SP).  F is never written.
//   k_batch_backward  G = B^T (A - 1)  (m x SP, reduction over the cells): 256 buffer columns x a contiguous row range per
//                     workgroup, the buffer tile staged k-major as it lies in memory; per-range partials, summed in range
//                     order by k_batch_sum.  (Both live in objective_batch.h: mln_dim_objective_batch uses them too.)
//
// Both kernels stream the buffer (HBM-bound at 2 n m 8 bytes per call) and spend 2 x 2 n m SP flop on the matrix cores.
// Every sum has a fixed order: two calls give identical bits.
//
// Layouts: every handle is batched -- explicit L, implicit (the buffer holds K = cov(x, xu): W = Lp^-T Z^T before,
// Lp^-1 G after, the block triangular solves with SP right-hand sides), Nystroem projections, mln_fit_from_L, the full
// GP (L = Lp, whose zero upper triangle is multiplied like any other entry), and any number of landmarks (no register-
// resident row, hence no 8192-column limit and no segmented route).  S > 64 is processed in chunks of 64 samples.
#include "api_internal.h"
#include "objective_batch.h"

namespace {

constexpr int S_CHUNK = 64;       // samples per launch (4 accumulator columns per wave)

template <int NT>
__global__ __launch_bounds__(256, 2) void k_batch_forward(const double* __restrict__ B, int64_t ldb, int64_t n, int64_t kdim,
                                                         const double* __restrict__ W, const double* __restrict__ V,
                                                         const double* __restrict__ Vdr, double mu, double* __restrict__ A1,
                                                         double* __restrict__ part_loss) {
  constexpr int SP = 16 * NT, WLD = SkinnyLd<NT>::v;
  __shared__ __attribute__((aligned(16))) double As[BT][A_LD];
  __shared__ double Ws[BK][WLD];
  __shared__ double lred[4][SP];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lk = lane >> 4, li = lane & 15;
  const int64_t r0 = (int64_t)blockIdx.x * BT;

  v4d acc[4][NT];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};

  d2 ra[8];
  double rw[NT];
  // buffer tile: 256 rows x 16 k; eight consecutive lanes read one row's 128 bytes (kdim = ldb is a multiple of 16)
  auto load_tiles = [&](int64_t k0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int idx = t + 256 * q;
      const int64_t gr = r0 + (idx >> 3);
      ra[q] = (gr < n) ? __builtin_nontemporal_load(reinterpret_cast<const d2*>(B + gr * ldb + k0) + (idx & 7)) : (d2){0.0, 0.0};
    }
#pragma unroll
    for (int q = 0; q < NT; ++q) rw[q] = W[k0 * SP + t + 256 * q];   // W has kdim rows (zero beyond m): 16 x SP contiguous
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
    for (int q = 0; q < NT; ++q) {
      const int idx = t + 256 * q;
      Ws[idx / SP][idx % SP] = rw[q];
    }
    __syncthreads();
    if (k0 + BK < kdim) load_tiles(k0 + BK);
#pragma unroll
    for (int kk = 0; kk < BK; kk += 4) {
      double a[4], b[NT];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = As[wave * 64 + i * 16 + li][kk + lk];
#pragma unroll
      for (int j = 0; j < NT; ++j) b[j] = Ws[kk + lk][j * 16 + li];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }
  // C/D layout of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * reg
  double ls[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) ls[j] = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = r0 + wave * 64 + i * 16 + lk + 4 * r;
      const bool ok = row < n;
      const int64_t rc = ok ? row : (n - 1);
      const double Vi = V[rc], Vd = Vdr[rc];
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const double f = acc[i][j][r] + mu;
        const double e = exp(f + Vi);
        if (ok) {
          ls[j] += (f + Vd) - e;                       // inference.py:89-91
          A1[row * SP + j * 16 + li] = e - 1.0;
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

// W[j][s] = Z[s][j] (ldl x SP, zero beyond m rows / S columns)
__global__ __launch_bounds__(256) void k_batch_z_to_w(const double* __restrict__ Z, int S, int64_t m, int SP, int64_t rows,
                                                      double* __restrict__ W) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * SP) return;
  const int64_t j = i / SP;
  const int s = (int)(i % SP);
  W[i] = (j < m && s < S) ? Z[(int64_t)s * m + j] : 0.0;
}

// prior terms, added once per sample (inference.py:45-46), and the gradient back in sample-major order:
//   loss[s] = lik[s] + 1/2 |z_s|^2 + (m/2) log 2 pi,  grad[s][j] = G[j][s] + z_s[j]
__global__ __launch_bounds__(256) void k_batch_finish(const double* __restrict__ Z, int64_t m, int SP,
                                                      const double* __restrict__ lik, const double* __restrict__ G,
                                                      double* __restrict__ loss, double* __restrict__ grad) {
  __shared__ double red[256];
  const int s = blockIdx.x, t = threadIdx.x;
  const double* z = Z + (int64_t)s * m;
  double zz = 0.0;
  for (int64_t j = t; j < m; j += 256) {
    const double v = z[j];
    zz = fma(v, v, zz);
    grad[(int64_t)s * m + j] = G[j * SP + s] + v;
  }
  red[t] = zz;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (t < off) red[t] += red[t + off];
    __syncthreads();
  }
  if (t == 0) loss[s] = lik[s] + 0.5 * red[0] + 0.5 * (double)m * 1.8378770664093453;   // log(2 pi)
}

template <int NT>
int launch_batch(mln_fit* f, const double* W, double* A1, double* part_loss, int64_t n_tiles, double* part, int n_ranges,
                 int64_t rows_per_range) {
  mln_ctx* ctx = f->ctx;
  hipLaunchKernelGGL((k_batch_forward<NT>), dim3((unsigned)n_tiles), dim3(256), 0, ctx->stream, f->L, f->ldl, f->n, f->ldl, W,
                     f->V, f->Vdr, f->mu, A1, part_loss);
  MLN_HIP(ctx, hipGetLastError());
  const unsigned col_blocks = (unsigned)((f->ldl + BT - 1) / BT);
  hipLaunchKernelGGL((k_batch_backward<NT>), dim3(col_blocks, (unsigned)n_ranges), dim3(256), 0, ctx->stream, f->L, f->ldl,
                     f->n, rows_per_range, A1, part);
  MLN_HIP(ctx, hipGetLastError());
  return MLN_OK;
}

}  // namespace

extern "C" int mln_objective_batch(mln_fit* f, const double* Z, int32_t S, double* loss, double* grad) {
  if (!f || !Z || !loss || !grad || S < 1) return MLN_ERR_ARG;
  mln_ctx* ctx = f->ctx;
  if (!f->V) { mln_set_error(ctx, "mln_fit_set_likelihood has not been called"); return MLN_ERR_ARG; }
  MLN_HIP(ctx, hipSetDevice(ctx->device));
  MLN_TRY(fit_ensure_lp(f));
  const int64_t m = f->m, ldl = f->ldl, n = f->n;
  const int sp_max = 16 * (int)((std::min<int64_t>(S, S_CHUNK) + 15) / 16);
  // row ranges of the backward kernel: about four workgroups per CU, at least 256 cells each
  const int64_t col_blocks = (ldl + BT - 1) / BT;
  const int64_t n_cu = ctx->n_cu > 0 ? ctx->n_cu : 256;
  int64_t n_ranges = std::max<int64_t>(1, (4 * n_cu) / col_blocks);
  n_ranges = std::min<int64_t>(n_ranges, std::max<int64_t>(1, (n + 255) / 256));
  const int64_t rows_per_range = std::max<int64_t>(16, (((n + n_ranges - 1) / n_ranges) + 15) / 16 * 16);
  const int64_t n_tiles = (n + BT - 1) / BT;
  // one block: Z chunk | W | [lik ; G] (all-reduced together) | a - 1 | likelihood partials | gradient partials | loss, grad out
  const size_t c_z = (size_t)sp_max * m, c_w = (size_t)ldl * sp_max, c_lg = (size_t)sp_max * (1 + ldl),
               c_a1 = (size_t)std::max<int64_t>(n, 1) * sp_max, c_pl = (size_t)std::max<int64_t>(n_tiles, 1) * sp_max,
               c_part = (size_t)n_ranges * ldl * sp_max, c_out = (size_t)sp_max * (1 + m);
  auto even = [](size_t c) { return (c + 1) & ~(size_t)1; };
  DevBuf<double> sc;
  MLN_TRY(sc.alloc(ctx, even(c_z) + even(c_w) + even(c_lg) + even(c_a1) + even(c_pl) + even(c_part) + even(c_out), "batched objective workspace"));
  double* d_Z = sc;
  double* d_W = d_Z + even(c_z);
  double* d_lg = d_W + even(c_w);
  double* d_A1 = d_lg + even(c_lg);
  double* d_pl = d_A1 + even(c_a1);
  double* d_part = d_pl + even(c_pl);
  double* d_out = d_part + even(c_part);

  for (int32_t s0 = 0; s0 < S; s0 += S_CHUNK) {
    const int Sc = std::min<int32_t>(S_CHUNK, S - s0);
    const int NT = (Sc + 15) / 16, SP = 16 * NT;
    double* d_lik = d_lg;
    double* d_G = d_lg + SP;
    MLN_HIP(ctx, hipMemcpyAsync(d_Z, Z + (int64_t)s0 * m, sizeof(double) * (size_t)Sc * m, hipMemcpyDefault, ctx->stream));
    hipLaunchKernelGGL(k_batch_z_to_w, dim3((unsigned)((ldl * SP + 255) / 256)), dim3(256), 0, ctx->stream, d_Z, Sc, m, SP, ldl, d_W);
    MLN_HIP(ctx, hipGetLastError());
    if (f->kspace) MLN_TRY(triinv_solve_left_T(ctx, f->tri, d_W, SP, SP));          // W = Lp^-T Z^T
    if (n > 0) {
      int rc = MLN_OK;
      switch (NT) {
        case 1: rc = launch_batch<1>(f, d_W, d_A1, d_pl, n_tiles, d_part, (int)n_ranges, rows_per_range); break;
        case 2: rc = launch_batch<2>(f, d_W, d_A1, d_pl, n_tiles, d_part, (int)n_ranges, rows_per_range); break;
        case 3: rc = launch_batch<3>(f, d_W, d_A1, d_pl, n_tiles, d_part, (int)n_ranges, rows_per_range); break;
        default: rc = launch_batch<4>(f, d_W, d_A1, d_pl, n_tiles, d_part, (int)n_ranges, rows_per_range); break;
      }
      MLN_TRY(rc);
      hipLaunchKernelGGL(k_batch_loss_sum, dim3((unsigned)SP), dim3(256), 0, ctx->stream, d_pl, n_tiles, SP, d_lik);
      MLN_HIP(ctx, hipGetLastError());
      hipLaunchKernelGGL(k_batch_sum, dim3((unsigned)((ldl * SP + 255) / 256)), dim3(256), 0, ctx->stream, d_part, (int)n_ranges, ldl * SP, d_G,
                         ldl * SP);
      MLN_HIP(ctx, hipGetLastError());
    } else {                                                                        // a rank without cells
      MLN_HIP(ctx, hipMemsetAsync(d_lg, 0, sizeof(double) * (size_t)SP * (1 + ldl), ctx->stream));
    }
    MLN_TRY(dev_allreduce(ctx, d_lg, (int64_t)SP * (1 + ldl)));
    if (f->kspace) MLN_TRY(triinv_solve_left(ctx, f->tri, d_G, SP, SP));            // L^T v = Lp^-1 (K^T v)
    double* o_loss = d_out;
    double* o_grad = d_out + SP;
    hipLaunchKernelGGL(k_batch_finish, dim3((unsigned)Sc), dim3(256), 0, ctx->stream, d_Z, m, SP, d_lik, d_G, o_loss, o_grad);
    MLN_HIP(ctx, hipGetLastError());
    MLN_HIP(ctx, hipMemcpyAsync(loss + s0, o_loss, sizeof(double) * (size_t)Sc, hipMemcpyDefault, ctx->stream));
    MLN_HIP(ctx, hipMemcpyAsync(grad + (int64_t)s0 * m, o_grad, sizeof(double) * (size_t)Sc * m, hipMemcpyDefault, ctx->stream));
    MLN_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return MLN_OK;
}
