// Predictive variances of a separable time-sensitive covariance on a whole time grid in one call.
//
// For cov((x,t),(c,s)) = k_state(x,c) k_time(t,s) the kernel row of query i at time t is the state row scaled column by
// column:  K_t[i,j] = Ks[i,j] S[t,j],  Ks = k_state(Xq, centres),  S[t,j] = k_time(t, s_j).  Per row chunk of r queries Ks is
// evaluated once; per block of T_b times the scaled rows are stacked into one tall panel
//   P[(t - t0) r + i][j] = Ks[i][j] S[t][j]                                   (k_stack_scaled_rows)
// and the chain the per-time entries run on r rows runs once on T_b r rows:
//   A = P Lf^-T                     triinv_solve_right_T, in place
//   cov [i,t] = kss[i] kdiag[t] - sum_q A[.,q]^2                              (k_row_sumsq_grid)
//   mcov[i,t] = sum_q std_q^2 A[.,q]^2        when W = Lf^-T diag(std): the same read of A, no second product
//             = sum_q (P W)[.,q]^2          general W (m x q): P regenerated (the solve destroyed it), one GEMM
//   cov [i,t] += base - (base - sum_q (P Cs^-T)[.,q]^2)                       the noisy landmark conditional's second factor
// Lf, Cs and W are uploaded once and each factor's TriInv is built once per call.
#include "api_internal.h"

namespace {

constexpr int STREAM_BLOCKS = 2048;   // 256 CUs x 8 blocks of 256 threads: a streaming kernel's grid; the rest is strided

// P[(t * r + i) * ld + j] = Ks[i * ld + j] * S[t * ld + j] for t < tb, i < r, j < m; columns m .. ld - 1 are zeros.
// Ks, S and P share the pitch ld (a multiple of 16, so every pair of columns is one aligned 16-byte access).  A thread
// owns pairs of columns of Ks rows (grid x) and writes them for every time of its slice (grid y).
__global__ __launch_bounds__(256) void k_stack_scaled_rows(const double* __restrict__ Ks, int64_t r, int64_t ld, int64_t m,
                                                           const double* __restrict__ S, int64_t tb,
                                                           double* __restrict__ P) {
  const int64_t ldh = ld >> 1;
  const int64_t pairs = r * ldh;
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < pairs; e += step) {
    const int64_t i = e / ldh;
    const int64_t j = (e - i * ldh) << 1;
    const double2 k = *reinterpret_cast<const double2*>(Ks + i * ld + j);
    for (int64_t t = blockIdx.y; t < tb; t += gridDim.y) {
      const double2 s = *reinterpret_cast<const double2*>(S + t * ld + j);
      double2 v;
      v.x = (j < m) ? k.x * s.x : 0.0;
      v.y = (j + 1 < m) ? k.y * s.y : 0.0;
      *reinterpret_cast<double2*>(P + (t * r + i) * ld + j) = v;
    }
  }
}

// One wave per panel row p = t * r + i (4 rows per block, rows strided over the grid): s = sum_{j < cols} A[p][j]^2 and,
// with column weights, sw = sum_j (w_j A[p][j])^2 from the same read.  With base = kss[i] kdiag[t] (0 without kss):
//   mode 0:  out_u[i * T + t]  = base + sign * s
//   mode 1:  out_u[i * T + t] += base - (base - s)
//   out_w[i * T + t] = sw
// The lanes' partial sums are combined in a fixed butterfly order: the same inputs give the same bits.
__global__ __launch_bounds__(256) void k_row_sumsq_grid(const double* __restrict__ A, int64_t ld, int64_t r, int64_t tb,
                                                        int64_t cols, const double* __restrict__ w,
                                                        const double* __restrict__ kss, const double* __restrict__ kdiag,
                                                        double sign, int mode, double* __restrict__ out_u,
                                                        double* __restrict__ out_w, int64_t T) {
  const int lane = threadIdx.x & 63;
  const int64_t rows = r * tb;
  const int64_t step = (int64_t)gridDim.x * 4;
  for (int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < rows; p += step) {
    const double* row = A + p * ld;
    double s = 0.0, sw = 0.0;
    for (int64_t j = 2 * lane; j < cols; j += 128) {
      const double2 v = *reinterpret_cast<const double2*>(row + j);
      const bool two = j + 1 < cols;
      s = fma(v.x, v.x, s);
      if (two) s = fma(v.y, v.y, s);
      if (w) {
        const double a = w[j] * v.x;
        sw = fma(a, a, sw);
        if (two) { const double b = w[j + 1] * v.y; sw = fma(b, b, sw); }
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      s += __shfl_xor(s, off, 64);
      sw += __shfl_xor(sw, off, 64);
    }
    if (lane == 0) {
      const int64_t t = p / r, i = p - t * r;
      const int64_t o = i * T + t;
      const double base = kss ? kss[i] * kdiag[t] : 0.0;
      if (out_u) out_u[o] = (mode == 0) ? base + sign * s : out_u[o] + (base - (base - s));
      if (out_w) out_w[o] = sw;
    }
  }
}

int launch_stack_scaled_rows(mln_ctx* ctx, const double* Ks, int64_t r, int64_t ld, int64_t m, const double* S, int64_t tb,
                             double* P) {
  const int64_t pairs = r * (ld / 2);
  const int64_t gx = std::min<int64_t>((pairs + 255) / 256, STREAM_BLOCKS);
  const int64_t gy = std::max<int64_t>(1, std::min<int64_t>(tb, STREAM_BLOCKS / gx));
  hipLaunchKernelGGL(k_stack_scaled_rows, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, ctx->stream, Ks, r, ld, m, S, tb, P);
  MLN_HIP(ctx, hipGetLastError());
  return MLN_OK;
}

int launch_row_sumsq_grid(mln_ctx* ctx, const double* A, int64_t ld, int64_t r, int64_t tb, int64_t cols, const double* w,
                          const double* kss, const double* kdiag, double sign, int mode, double* out_u, double* out_w,
                          int64_t T) {
  const int64_t g = std::min<int64_t>((r * tb + 3) / 4, STREAM_BLOCKS);
  hipLaunchKernelGGL(k_row_sumsq_grid, dim3((unsigned)g), dim3(256), 0, ctx->stream, A, ld, r, tb, cols, w, kss, kdiag, sign,
                     mode, out_u, out_w, T);
  MLN_HIP(ctx, hipGetLastError());
  return MLN_OK;
}

}  // namespace

// Chunking: with B = scratch_doubles (0: 2^27, 1 GiB), ld = pad16(m), ldq = pad16(q) for a general W (else 0), a row chunk
// holds Ks (r x ld) and a time block the panel (T_b r x ld) and the GEMM result (T_b r x ldq):
//   r   = B / (2 ld + ldq) rounded down to a multiple of 64, within [64, min(32768, n rounded up to 64)]
//   T_b = (B - r ld) / (r (ld + ldq)), within [1, T]
// -- never fewer than 64 rows or one time, whatever B says.
extern "C" int mln_predict_variance_grid(mln_ctx* ctx, const mln_kernel_desc* state, const double* xq, int64_t n, int32_t d,
                                         const double* centers, int64_t m, const double* S, int64_t T, const double* kdiag,
                                         const double* Lf, const double* Cs, const double* W, int64_t q, const double* w_std,
                                         int64_t scratch_doubles, double* cov_out, double* mcov_out) {
  if (!ctx) return MLN_ERR_ARG;
  if (n < 0 || T < 0 || m < 1 || d < 1 || (W && q < 1) || scratch_doubles < 0) { mln_set_error(ctx, "bad shape"); return MLN_ERR_SHAPE; }
  if (!cov_out && !mcov_out) { mln_set_error(ctx, "variance grid: no output requested"); return MLN_ERR_ARG; }
  if (W && w_std) { mln_set_error(ctx, "variance grid: W and std exclude each other"); return MLN_ERR_ARG; }
  if (mcov_out && !W && !w_std) { mln_set_error(ctx, "variance grid: the mean covariance needs W or std"); return MLN_ERR_ARG; }
  if (n == 0 || T == 0) return MLN_OK;
  const bool use_l = cov_out || (mcov_out && w_std);   // the Lf solve serves the covariance and the std route
  const bool use_cs = cov_out && Cs;
  const bool use_w = mcov_out && W;
  if (!xq || !centers || !S || (cov_out && !kdiag) || (use_l && !Lf)) return MLN_ERR_ARG;
  MLN_HIP(ctx, hipSetDevice(ctx->device));
  DevCov dc;
  MLN_TRY(mln_lower_cov(ctx, state, d, &dc));
  const int64_t ld = pad16(m), ldq = use_w ? pad16(q) : 0;
  const int64_t budget = scratch_doubles ? scratch_doubles : ((int64_t)1 << 27);
  const int64_t r_max = std::min<int64_t>(32768, ((n + 63) / 64) * 64);
  int64_t r = (budget / (2 * ld + ldq) / 64) * 64;
  r = std::max<int64_t>(64, std::min(r, r_max));
  int64_t tb = (budget - r * ld) / (r * (ld + ldq));
  tb = std::max<int64_t>(1, std::min(tb, T));

  DevIn dx, dcen, dl, dcs, dw, dstd, dkd, ds;
  DevOut oc, om;
  MLN_TRY(dx.init(ctx, xq, (size_t)n * d));
  MLN_TRY(dcen.init(ctx, centers, (size_t)m * d));
  if (use_l) MLN_TRY(dl.init(ctx, Lf, (size_t)m * m));
  if (use_cs) MLN_TRY(dcs.init(ctx, Cs, (size_t)m * m));
  if (use_w) MLN_TRY(dw.init(ctx, W, (size_t)m * q));
  if (mcov_out && w_std) MLN_TRY(dstd.init(ctx, w_std, (size_t)m));
  if (cov_out) MLN_TRY(dkd.init(ctx, kdiag, (size_t)T));
  MLN_TRY(ds.init(ctx, S, (size_t)T * m));
  MLN_TRY(oc.init(ctx, cov_out, cov_out ? (size_t)n * T : 0));
  MLN_TRY(om.init(ctx, mcov_out, mcov_out ? (size_t)n * T : 0));

  // S at the panel's pitch, pad columns zero: the stacking kernel reads it in aligned pairs
  DevBuf<double> Sp, Ks, P, G, kss;
  MLN_TRY(Sp.alloc_zeroed(ctx, (size_t)T * ld, "Sp"));
  MLN_HIP(ctx, hipMemcpy2DAsync(Sp, sizeof(double) * (size_t)ld, ds.dev, sizeof(double) * (size_t)m, sizeof(double) * (size_t)m,
                                (size_t)T, hipMemcpyDeviceToDevice, ctx->stream));
  TriInv tl, tc;
  if (use_l) MLN_TRY(triinv_build(ctx, dl.dev, m, m, true, false, &tl));
  if (use_cs) MLN_TRY(triinv_build(ctx, dcs.dev, m, m, true, false, &tc));
  int rc = Ks.alloc(ctx, (size_t)r * ld, "Ks");
  if (rc == MLN_OK) rc = P.alloc(ctx, (size_t)tb * r * ld, "P");
  if (rc == MLN_OK && use_w) rc = G.alloc(ctx, (size_t)tb * r * ldq, "G");
  if (rc == MLN_OK && cov_out) rc = kss.alloc(ctx, (size_t)r, "kss");
  for (int64_t r0 = 0; r0 < n && rc == MLN_OK; r0 += r) {
    const int64_t rows = std::min(r, n - r0);
    rc = launch_kernel_matrix(ctx, dc, dx.dev + r0 * d, rows, dcen.dev, m, d, Ks, ld, 0.0);
    if (rc == MLN_OK && cov_out) rc = launch_cov_diag(ctx, dc, dx.dev + r0 * d, rows, d, kss);
    for (int64_t t0 = 0; t0 < T && rc == MLN_OK; t0 += tb) {
      const int64_t nt = std::min(tb, T - t0);
      const double* St = Sp + t0 * ld;
      double* co = cov_out ? oc.dev + r0 * T + t0 : nullptr;
      double* mo = mcov_out ? om.dev + r0 * T + t0 : nullptr;
      if (use_l) {
        rc = launch_stack_scaled_rows(ctx, Ks, rows, ld, m, St, nt, P);
        if (rc == MLN_OK) rc = triinv_solve_right_T(ctx, tl, P, nt * rows, ld);
        if (rc == MLN_OK)
          rc = launch_row_sumsq_grid(ctx, P, ld, rows, nt, m, w_std ? dstd.dev : nullptr, cov_out ? kss.get() : nullptr,
                                     cov_out ? dkd.dev + t0 : nullptr, -1.0, 0, co, w_std ? mo : nullptr, T);
      }
      if (rc == MLN_OK && use_cs) {
        rc = launch_stack_scaled_rows(ctx, Ks, rows, ld, m, St, nt, P);
        if (rc == MLN_OK) rc = triinv_solve_right_T(ctx, tc, P, nt * rows, ld);
        if (rc == MLN_OK) rc = launch_row_sumsq_grid(ctx, P, ld, rows, nt, m, nullptr, kss, dkd.dev + t0, 1.0, 1, co, nullptr, T);
      }
      if (rc == MLN_OK && use_w) {
        rc = launch_stack_scaled_rows(ctx, Ks, rows, ld, m, St, nt, P);
        GemmArgs g{};
        g.A = P; g.lda = ld; g.B = dw.dev; g.ldb = q; g.C = G; g.ldc = ldq;
        g.M = nt * rows; g.N = q; g.K = m; g.alpha = 1.0; g.beta = 0.0; g.ta = 0; g.tb = 0;
        if (rc == MLN_OK) rc = launch_dgemm(ctx, g);
        if (rc == MLN_OK) rc = launch_row_sumsq_grid(ctx, G, ldq, rows, nt, q, nullptr, nullptr, nullptr, 1.0, 0, mo, nullptr, T);
      }
    }
  }
  if (rc == MLN_OK && cov_out) rc = oc.commit();
  if (rc == MLN_OK && mcov_out) rc = om.commit();
  (void)hipStreamSynchronize(ctx->stream);
  return rc;
}
