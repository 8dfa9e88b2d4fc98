// Derivatives of block-evaluated covariance trees (more than MLN_MAX_LEAVES leaves, deeper than one device program's
// stack, or with user-defined leaves): the device side of mellon_amd/block_derivatives.py.
//
// For one pair (x_i, c_j) the covariance is P(k_1 .. k_L) over its leaves (reference base_cov.py:317-497 carries k_grad
// through Add / Mul / Pow; base_predictor.py:490-539 differentiates `_mean`).  With a_l = dP/dk_l, a_ll' = d2P/dk_l dk_l',
// leaf gradients  grad k_l = gam_l (sig_l x - c)|dims_l  (stationary: gam = g, sig = 1; Linear: gam = -1/ls, sig = 0) and
// leaf Hessians  g_l I|dims_l + h_l (x - c)(x - c)^T|dims_l:
//   grad_i = sum_j w_j sum_l a_l grad k_l
//   H_i    = sum_j w_j [ sum_l a_l g_l I_l + sum_l (a_l h_l + a_ll gam_l^2) dl dl^T
//                        + sum_{l<l'} a_ll' gam_l gam_l' (dl dl'^T + dl' dl^T) ]
// -- the formula above k_hess_coeff (cov_kernels.hip); there a_l / a_ll' come from program_adjoints / program_second in
// registers, here the binding propagates them through a tree of any size as (rows x ld) blocks (mln_ewise) and hands the
// products in:
//   mln_leaf_factors           K, g (and h) blocks of ONE built-in leaf: the tile pass of k_grad_coeff_multi / k_hess_coeff,
//                              calling the same leaf_value / leaf_grad_coeff / leaf_hess_coeff / leaf_value_grad (cov_leaf.h)
//   mln_block_grad_accumulate  per leaf one GEMM  T = Q_l [w C|dims_l, w]  and the expansion x T_nd - T_k
//   mln_block_hess_accumulate  per leaf a weighted row sum onto the diagonal, per leaf pair one GEMM against
//                              w [vec(c_l c_l'^T) | c_l | c_l' | 1] and the expansion of (sig x - c)(sig' x - c)^T
//   mln_block_kernel_grad      out[i][j][:] = sum_l A_l,ij (y_j - x_i)|dims_l   (Linear: A_l,ij x_i|dims_l)
// The weights multiply the CENTRE operand of each GEMM (sum_j Q_ij w_j c_j), so the coefficient blocks carry no w.
#include <vector>

#include "api_internal.h"
#include "cov_leaf.h"

namespace {

constexpr int TM = covtile::TM, TN = covtile::TN, DK = covtile::DK, PADT = covtile::PADT;

// K / g / h (rows x ld) of one leaf; columns m .. ld - 1 are written as zeros, rows and columns past the edges masked.
__global__ __launch_bounds__(256) void k_leaf_factors(DevCov cov, const double* __restrict__ x, int64_t n,
                                                      const double* __restrict__ y, int64_t m, int d,
                                                      const double* __restrict__ xx, const double* __restrict__ yy,
                                                      int exact_denominator, double* __restrict__ K,
                                                      double* __restrict__ g, double* __restrict__ h, int64_t ld,
                                                      int64_t tiles_n) {
  __shared__ double xs[DK][TM + PADT];
  __shared__ double ys[DK][TN + PADT];
  const int64_t bid = blockIdx.x;
  const int64_t row0 = (bid / tiles_n) * TM, col0 = (bid % tiles_n) * TN;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const DevLeaf lf = cov.leaves[0];
  double acc[4][4], xr[4], yr[4];
  leaf_dot(cov, lf, x, n, y, m, d, row0, col0, xs, ys, acc);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t r = row0 + ty * 4 + i;
    xr[i] = (r < n) ? xx[r] : 0.0;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t c = col0 + tx * 4 + j;
    yr[j] = (c < m) ? yy[c] : 0.0;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t r = row0 + ty * 4 + i;
    if (r >= n) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t c = col0 + tx * 4 + j;
      if (c >= ld) continue;
      double kv = 0.0, gv = 0.0, hv = 0.0;
      if (c < m) {
        if (lf.kind == MLN_K_LINEAR || !exact_denominator) {
          leaf_value_grad(lf, xr[i], yr[j], acc[i][j], exact_denominator, &kv, &gv);
        } else {
          kv = leaf_value(lf, xr[i], yr[j], acc[i][j]);
          gv = leaf_grad_coeff(lf, xr[i], yr[j], acc[i][j]);
        }
        if (h) hv = leaf_hess_coeff(lf, xr[i], yr[j], acc[i][j]);
      }
      const int64_t at = r * ld + c;
      K[at] = kv;
      g[at] = gv;
      if (h) h[at] = hv;
    }
  }
}

// Cext[j][k] = w_j c_j[dims[k]] (k < nd), Cext[j][nd] = w_j, zero up to ldc
__global__ void k_bd_grad_centres(const int* __restrict__ dims, int nd, const double* __restrict__ c, int64_t m, int d,
                                  const double* __restrict__ w, double* __restrict__ cext, int64_t ldc) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= m * ldc) return;
  const int64_t j = idx / ldc;
  const int k = (int)(idx % ldc);
  double v = 0.0;
  if (k < nd) v = w[j] * c[j * d + dims[k]];
  else if (k == nd) v = w[j];
  cext[idx] = v;
}

// stationary: out[i][dims[k]] += x_i[dims[k]] T_i,nd - T_i,k ; Linear: out[i][dims[k]] += T_i,k
__global__ void k_bd_grad_combine(const int* __restrict__ dims, int nd, int linear, const double* __restrict__ T,
                                  int64_t ldt, const double* __restrict__ x, int64_t rows, int d,
                                  double* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * nd) return;
  const int64_t i = idx / nd;
  const int k = (int)(idx % nd);
  const int dim = dims[k];
  out[i * d + dim] += linear ? T[i * ldt + k] : x[i * d + dim] * T[i * ldt + nd] - T[i * ldt + k];
}

// Cp[j] = w_j [ c_j[da[a]] c_j[db[b]] (a * nb + b) | c_j[da[a]] | c_j[db[b]] | 1 ], zero up to ldc
__global__ void k_bd_hess_centres(const int* __restrict__ da, int na, const int* __restrict__ db, int nb,
                                  const double* __restrict__ c, int64_t m, int d, const double* __restrict__ w,
                                  double* __restrict__ cp, int64_t ldc) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= m * ldc) return;
  const int64_t j = idx / ldc;
  const int k = (int)(idx % ldc);
  const double* cj = c + j * d;
  double v = 0.0;
  if (k < na * nb) v = cj[da[k / nb]] * cj[db[k % nb]];
  else if (k < na * nb + na) v = cj[da[k - na * nb]];
  else if (k < na * nb + na + nb) v = cj[db[k - na * nb - na]];
  else if (k == na * nb + na + nb) v = 1.0;
  cp[idx] = v * w[j];
}

// H_i[da[a]][db[b]] (transpose = 0) or H_i[db[b]][da[a]] (transpose = 1)
//   += sig sig' s x_a x_b - sig x_a (Q c')_b - sig' (Q c)_a x_b + (Q c c'^T)_ab
__global__ void k_bd_hess_combine(const int* __restrict__ dims_a, int na, double sa, const int* __restrict__ dims_b,
                                  int nb, double sb, int transpose, const double* __restrict__ T, int64_t ldt,
                                  const double* __restrict__ x, int64_t rows, int d, double* __restrict__ H) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * na * nb) return;
  const int64_t i = idx / (na * nb);
  const int ab = (int)(idx % (na * nb)), a = ab / nb, b = ab % nb;
  const int da = dims_a[a], db = dims_b[b];
  const double* Ti = T + i * ldt;
  const double xa = x[i * d + da], xb = x[i * d + db];
  const double val = sa * sb * Ti[na * nb + na + nb] * xa * xb - sa * xa * Ti[na * nb + na + b]
                     - sb * Ti[na * nb + a] * xb + Ti[ab];
  double* Hi = H + i * (int64_t)d * d;
  if (transpose) Hi[db * d + da] += val; else Hi[da * d + db] += val;
}

// H_i[dim][dim] += sum_j w_j Qd[i][j] for the dims of one stationary leaf (one workgroup per row)
__global__ __launch_bounds__(256) void k_bd_hess_diag(const int* __restrict__ dims, int nd,
                                                      const double* __restrict__ Qd, int64_t ldq, int64_t m,
                                                      const double* __restrict__ w, int64_t rows, int d,
                                                      double* __restrict__ H) {
  __shared__ double red[256];
  const int64_t i = blockIdx.x;
  if (i >= rows) return;
  double s = 0.0;
  for (int64_t j = threadIdx.x; j < m; j += 256) s = fma(Qd[i * ldq + j], w[j], s);
  red[threadIdx.x] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  for (int k = threadIdx.x; k < nd; k += 256) {
    const int dim = dims[k];
    H[i * (int64_t)d * d + (int64_t)dim * d + dim] += red[0];
  }
}

struct BdLeafMeta { int kind, ndims, dims_off, pad; };

// out[i][j][:] = sum_l A_l[i][j] (y_j - x_i)|dims_l  (Linear: A_l[i][j] x_i|dims_l); one thread per pair
__global__ void k_bd_kernel_grad(const BdLeafMeta* __restrict__ meta, int L, const int* __restrict__ dims,
                                 const double* const* __restrict__ A, int64_t ld, const double* __restrict__ x,
                                 int64_t n, const double* __restrict__ y, int64_t m, int d, double* __restrict__ out) {
  const int64_t total = n * m;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = idx / m, j = idx % m;
    const double* xi = x + i * d;
    const double* yj = y + j * d;
    double* o = out + idx * d;
    for (int dim = 0; dim < d; ++dim) o[dim] = 0.0;
    for (int l = 0; l < L; ++l) {
      const BdLeafMeta lf = meta[l];
      const double a = A[l][i * ld + j];
      for (int k = 0; k < lf.ndims; ++k) {
        const int dim = dims[lf.dims_off + k];
        o[dim] += (lf.kind == MLN_K_LINEAR) ? a * xi[dim] : a * (yj[dim] - xi[dim]);
      }
    }
  }
}

// The leaf list of one call on the device: every leaf's column indices in one int array.
struct LeafList {
  std::vector<BdLeafMeta> meta;
  std::vector<int> dims_h;
  DevBuf<int> dims;
  int nd_max = 0;
  int init(mln_ctx* ctx, const mln_leaf* leaves, int L, int d) {
    if (!leaves || L < 1) { mln_set_error(ctx, "block derivatives: empty leaf list"); return MLN_ERR_ARG; }
    for (int l = 0; l < L; ++l) {
      const mln_leaf& lf = leaves[l];
      if (lf.kind < MLN_K_MATERN32 || lf.kind > MLN_K_LINEAR) {
        mln_set_error(ctx, "block derivatives: leaf kind without derivatives");
        return MLN_ERR_UNSUPPORTED;
      }
      if (lf.ndims < 1 || !lf.dims) { mln_set_error(ctx, "block derivatives: leaf without active columns"); return MLN_ERR_ARG; }
      meta.push_back(BdLeafMeta{lf.kind, lf.ndims, (int)dims_h.size(), 0});
      for (int k = 0; k < lf.ndims; ++k) {
        if (lf.dims[k] < 0 || lf.dims[k] >= d) { mln_set_error(ctx, "block derivatives: active column out of range"); return MLN_ERR_SHAPE; }
        dims_h.push_back(lf.dims[k]);
      }
      if (lf.ndims > nd_max) nd_max = lf.ndims;
    }
    MLN_TRY(dims.alloc(ctx, dims_h.size(), "leaf columns"));
    MLN_HIP(ctx, hipMemcpyAsync(dims, dims_h.data(), sizeof(int) * dims_h.size(), hipMemcpyHostToDevice, ctx->stream));
    MLN_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MLN_OK;
  }
  const int* dims_of(int l) const { return dims.get() + meta[l].dims_off; }
};

int check_blocks(mln_ctx* ctx, const double* const* blocks, int count, bool nullable) {
  for (int b = 0; b < count; ++b) {
    if (!blocks[b]) {
      if (nullable) continue;
      mln_set_error(ctx, "block derivatives: missing coefficient block");
      return MLN_ERR_ARG;
    }
    if (!is_device_ptr(blocks[b])) { mln_set_error(ctx, "block derivatives: coefficient blocks live on the device"); return MLN_ERR_ARG; }
  }
  return MLN_OK;
}

}  // namespace

extern "C" int mln_leaf_factors(mln_ctx* ctx, const mln_kernel_desc* leaf, const double* x, int64_t n, const double* y,
                                int64_t m, int32_t d, int32_t exact_denominator, int64_t ld, double* K, double* g,
                                double* h) {
  if (!ctx) return MLN_ERR_ARG;
  if (n < 0 || m < 0 || d < 1 || ld < m) { mln_set_error(ctx, "bad shape"); return MLN_ERR_SHAPE; }
  if (n == 0 || m == 0) return MLN_OK;
  if (!leaf || !x || !y || !K || !g) return MLN_ERR_ARG;
  if (leaf->n_leaves != 1 || leaf->n_toks != 1) { mln_set_error(ctx, "mln_leaf_factors takes a one-leaf descriptor"); return MLN_ERR_ARG; }
  MLN_HIP(ctx, hipSetDevice(ctx->device));
  DevCov dc;
  MLN_TRY(mln_lower_cov(ctx, leaf, d, &dc));
  MLN_TRY(reject_distance_leaf(ctx, dc));
  DevIn dx, dy;
  DevOut oK, og, oh;
  MLN_TRY(dx.init(ctx, x, (size_t)n * d));
  MLN_TRY(dy.init(ctx, y, (size_t)m * d));
  MLN_TRY(oK.init(ctx, K, (size_t)n * ld));
  MLN_TRY(og.init(ctx, g, (size_t)n * ld));
  if (h) MLN_TRY(oh.init(ctx, h, (size_t)n * ld));
  DevBuf<double> norms;
  MLN_TRY(norms.alloc(ctx, (size_t)(n + m), "norms"));
  MLN_TRY(launch_leaf_sqnorms(ctx, dc, dx.dev, n, d, norms));
  MLN_TRY(launch_leaf_sqnorms(ctx, dc, dy.dev, m, d, norms + n));
  const int64_t tiles_n = (ld + TN - 1) / TN, nblk = tiles_n * ((n + TM - 1) / TM);
  if (nblk > 0x7fffffffLL) { mln_set_error(ctx, "leaf factors: block too large for one launch"); return MLN_ERR_UNSUPPORTED; }
  hipLaunchKernelGGL(k_leaf_factors, dim3((unsigned)nblk), dim3(256), 0, ctx->stream, dc, dx.dev, n, dy.dev, m, (int)d,
                     norms.get(), norms.get() + n, (int)exact_denominator, oK.dev, og.dev, h ? oh.dev : nullptr, ld, tiles_n);
  MLN_HIP(ctx, hipGetLastError());
  MLN_TRY(oK.commit());
  MLN_TRY(og.commit());
  if (h) MLN_TRY(oh.commit());
  return MLN_OK;
}

extern "C" int mln_block_grad_accumulate(mln_ctx* ctx, const mln_leaf* leaves, int32_t n_leaves, const double* const* Q,
                                         int64_t ld, const double* x, int64_t n, int32_t d, const double* centers,
                                         int64_t m, const double* w, double* out) {
  if (!ctx) return MLN_ERR_ARG;
  if (n < 0 || m < 1 || d < 1 || ld < m) { mln_set_error(ctx, "bad shape"); return MLN_ERR_SHAPE; }
  if (n == 0) return MLN_OK;
  if (!Q || !x || !centers || !w || !out) return MLN_ERR_ARG;
  MLN_HIP(ctx, hipSetDevice(ctx->device));
  LeafList ll;
  MLN_TRY(ll.init(ctx, leaves, n_leaves, d));
  MLN_TRY(check_blocks(ctx, Q, n_leaves, false));
  DevIn dx, dc_, dw;
  DevOut o;
  MLN_TRY(dx.init(ctx, x, (size_t)n * d));
  MLN_TRY(dc_.init(ctx, centers, (size_t)m * d));
  MLN_TRY(dw.init(ctx, w, (size_t)m));
  MLN_TRY(o.init(ctx, out, (size_t)n * d));
  const int64_t ldc = pad16(ll.nd_max + 1);
  DevBuf<double> T, cext;
  MLN_TRY(T.alloc(ctx, (size_t)n * ldc, "T"));
  MLN_TRY(cext.alloc(ctx, (size_t)m * ldc, "cext"));
  MLN_HIP(ctx, hipMemsetAsync(o.dev, 0, sizeof(double) * (size_t)n * d, ctx->stream));
  int rc = MLN_OK;
  for (int l = 0; l < n_leaves && rc == MLN_OK; ++l) {
    const int nd = ll.meta[l].ndims;
    hipLaunchKernelGGL(k_bd_grad_centres, dim3((unsigned)((m * ldc + 255) / 256)), dim3(256), 0, ctx->stream,
                       ll.dims_of(l), nd, dc_.dev, m, (int)d, dw.dev, cext.get(), ldc);
    GemmArgs g{};
    g.A = Q[l]; g.lda = ld; g.ta = 0; g.B = cext; g.ldb = ldc; g.tb = 0; g.C = T; g.ldc = ldc;
    g.M = n; g.N = nd + 1; g.K = m; g.alpha = 1.0; g.beta = 0.0; g.split_k = 1;
    rc = launch_dgemm(ctx, g);
    if (rc != MLN_OK) break;
    hipLaunchKernelGGL(k_bd_grad_combine, dim3((unsigned)((n * nd + 255) / 256)), dim3(256), 0, ctx->stream,
                       ll.dims_of(l), nd, ll.meta[l].kind == MLN_K_LINEAR ? 1 : 0, T.get(), ldc, dx.dev, n, (int)d, o.dev);
  }
  hipError_t e = hipGetLastError();
  if (rc == MLN_OK && e != hipSuccess) rc = mln_hip_fail(ctx, e, "block_grad_accumulate", __FILE__, __LINE__);
  if (rc == MLN_OK) rc = o.commit();
  (void)hipStreamSynchronize(ctx->stream);
  return rc;
}

extern "C" int mln_block_hess_accumulate(mln_ctx* ctx, const mln_leaf* leaves, int32_t n_leaves, const double* const* Qd,
                                         const double* const* Qp, int64_t ld, const double* x, int64_t n, int32_t d,
                                         const double* centers, int64_t m, const double* w, double* out) {
  if (!ctx) return MLN_ERR_ARG;
  if (n < 0 || m < 1 || d < 1 || ld < m) { mln_set_error(ctx, "bad shape"); return MLN_ERR_SHAPE; }
  if (n == 0) return MLN_OK;
  if (!Qd || !Qp || !x || !centers || !w || !out) return MLN_ERR_ARG;
  MLN_HIP(ctx, hipSetDevice(ctx->device));
  const int L = n_leaves;
  LeafList ll;
  MLN_TRY(ll.init(ctx, leaves, L, d));
  MLN_TRY(check_blocks(ctx, Qd, L, true));
  MLN_TRY(check_blocks(ctx, Qp, (L * (L + 1)) / 2, true));
  DevIn dx, dc_, dw;
  DevOut o;
  MLN_TRY(dx.init(ctx, x, (size_t)n * d));
  MLN_TRY(dc_.init(ctx, centers, (size_t)m * d));
  MLN_TRY(dw.init(ctx, w, (size_t)m));
  MLN_TRY(o.init(ctx, out, (size_t)n * d * d));
  const int64_t ldt = pad16((int64_t)ll.nd_max * ll.nd_max + 2 * ll.nd_max + 1);
  DevBuf<double> T, cp;
  MLN_TRY(T.alloc(ctx, (size_t)n * ldt, "T"));
  MLN_TRY(cp.alloc(ctx, (size_t)m * ldt, "cp"));
  MLN_HIP(ctx, hipMemsetAsync(o.dev, 0, sizeof(double) * (size_t)n * d * d, ctx->stream));
  int rc = MLN_OK;
  int slot = 0;
  for (int l = 0; l < L && rc == MLN_OK; ++l) {
    const int na = ll.meta[l].ndims;
    const double sa = ll.meta[l].kind == MLN_K_LINEAR ? 0.0 : 1.0;
    if (Qd[l] && ll.meta[l].kind != MLN_K_LINEAR)
      hipLaunchKernelGGL(k_bd_hess_diag, dim3((unsigned)n), dim3(256), 0, ctx->stream, ll.dims_of(l), na, Qd[l], ld, m,
                         dw.dev, n, (int)d, o.dev);
    for (int lp = l; lp < L && rc == MLN_OK; ++lp, ++slot) {
      if (!Qp[slot]) continue;
      const int nb = ll.meta[lp].ndims;
      const double sb = ll.meta[lp].kind == MLN_K_LINEAR ? 0.0 : 1.0;
      const int64_t ncol = (int64_t)na * nb + na + nb + 1, ldc = pad16(ncol);
      hipLaunchKernelGGL(k_bd_hess_centres, dim3((unsigned)((m * ldc + 255) / 256)), dim3(256), 0, ctx->stream,
                         ll.dims_of(l), na, ll.dims_of(lp), nb, dc_.dev, m, (int)d, dw.dev, cp.get(), ldc);
      GemmArgs g{};
      g.A = Qp[slot]; g.lda = ld; g.ta = 0; g.B = cp; g.ldb = ldc; g.tb = 0; g.C = T; g.ldc = ldc;
      g.M = n; g.N = ncol; g.K = m; g.alpha = 1.0; g.beta = 0.0; g.split_k = 1;
      rc = launch_dgemm(ctx, g);
      if (rc != MLN_OK) break;
      const unsigned nb_ = (unsigned)((n * na * nb + 255) / 256);
      hipLaunchKernelGGL(k_bd_hess_combine, dim3(nb_), dim3(256), 0, ctx->stream, ll.dims_of(l), na, sa, ll.dims_of(lp),
                         nb, sb, 0, T.get(), ldc, dx.dev, n, (int)d, o.dev);
      if (lp != l)
        hipLaunchKernelGGL(k_bd_hess_combine, dim3(nb_), dim3(256), 0, ctx->stream, ll.dims_of(l), na, sa,
                           ll.dims_of(lp), nb, sb, 1, T.get(), ldc, dx.dev, n, (int)d, o.dev);
    }
  }
  hipError_t e = hipGetLastError();
  if (rc == MLN_OK && e != hipSuccess) rc = mln_hip_fail(ctx, e, "block_hess_accumulate", __FILE__, __LINE__);
  if (rc == MLN_OK) rc = o.commit();
  (void)hipStreamSynchronize(ctx->stream);
  return rc;
}

extern "C" int mln_block_kernel_grad(mln_ctx* ctx, const mln_leaf* leaves, int32_t n_leaves, const double* const* A,
                                     int64_t ld, const double* x, int64_t n, const double* y, int64_t m, int32_t d,
                                     double* out) {
  if (!ctx) return MLN_ERR_ARG;
  if (n < 0 || m < 0 || d < 1 || ld < m) { mln_set_error(ctx, "bad shape"); return MLN_ERR_SHAPE; }
  if (n == 0 || m == 0) return MLN_OK;
  if (!A || !x || !y || !out) return MLN_ERR_ARG;
  MLN_HIP(ctx, hipSetDevice(ctx->device));
  LeafList ll;
  MLN_TRY(ll.init(ctx, leaves, n_leaves, d));
  MLN_TRY(check_blocks(ctx, A, n_leaves, false));
  DevIn dx, dy;
  DevOut o;
  MLN_TRY(dx.init(ctx, x, (size_t)n * d));
  MLN_TRY(dy.init(ctx, y, (size_t)m * d));
  MLN_TRY(o.init(ctx, out, (size_t)n * m * d));
  DevBuf<BdLeafMeta> meta;
  DevBuf<const double*> ptrs;
  MLN_TRY(meta.alloc(ctx, (size_t)n_leaves, "leaf list"));
  MLN_TRY(ptrs.alloc(ctx, (size_t)n_leaves, "block pointers"));
  MLN_HIP(ctx, hipMemcpyAsync(meta, ll.meta.data(), sizeof(BdLeafMeta) * (size_t)n_leaves, hipMemcpyHostToDevice, ctx->stream));
  MLN_HIP(ctx, hipMemcpyAsync(ptrs, A, sizeof(const double*) * (size_t)n_leaves, hipMemcpyHostToDevice, ctx->stream));
  MLN_HIP(ctx, hipStreamSynchronize(ctx->stream));
  int64_t blocks = (n * m + 255) / 256;
  if (blocks > 65535 * 16) blocks = 65535 * 16;
  hipLaunchKernelGGL(k_bd_kernel_grad, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, meta.get(), (int)n_leaves,
                     ll.dims.get(), ptrs.get(), ld, dx.dev, n, dy.dev, m, (int)d, o.dev);
  MLN_HIP(ctx, hipGetLastError());
  return o.commit();
}
