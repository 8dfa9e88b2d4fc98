// Gradient and Hessian of the predictive mean through the matrix cores, fp64, gfx950 (Predictor.gradient / hessian,
// mellon/base_predictor.py:490-521, which the reference obtains with jax.jacrev / jacfwd of `_mean`).  One driver per
// derivative order (gradient_pass, hessian_pass) serves every route -- one output or p, weights in the coefficient matrices
// or in the centre operands, Hessians returned or factored in scratch:
//   per row chunk:                            ONE covariance-tile pass writes the coefficient matrices Q
//   per output block, per leaf / leaf pair:   the centre operand Z, ONE GEMM T = Q Z, the expansion of T into the result
// The tile layout is that of cov_kernels.hip (64 x 64 per workgroup, 4 x 4 outputs per thread).
#include <cstdlib>

#include "mln_internal.h"
#include "cov_tile.h"
#include "linalg.h"

namespace {

constexpr int TM = covtile::TM, TN = covtile::TN, DK = covtile::DK, PADT = covtile::PADT;

// ---- predictor gradient, single stationary leaf: grad_i = sum_j w_j g_ij (x_i - c_j)|dims -------------------
//   Q (rows x m) = w_j g_ij                     one covariance-tile pass (this kernel; w == nullptr: Q = g_ij, the
//                                               weight-less form of the p-output route below)
//   T = Q [C|dims , 1]                          one GEMM on the matrix cores
//   grad_i[dims] = x_i[dims] T_i,last - T_i,k   (k_grad_combine_outputs)
__global__ __launch_bounds__(256) void k_grad_coeff(DevCov cov, const double* __restrict__ x, int64_t n,
                                                    const double* __restrict__ y, int64_t m, int d,
                                                    const double* __restrict__ xx, const double* __restrict__ yy,
                                                    const double* __restrict__ w, double* __restrict__ out,
                                                    int64_t ldo, int64_t tiles_n) {
  __shared__ double xs[DK][TM + PADT];
  __shared__ double ys[DK][TN + PADT];
  const int64_t bid = blockIdx.x;
  const int64_t row0 = (bid / tiles_n) * TM, col0 = (bid % tiles_n) * TN;
  double val[4][4];
  cov_tile<true, true>(cov, x, n, y, m, d, xx, yy, row0, col0, xs, ys, val);
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t r = row0 + ty * 4 + i;
    if (r >= n) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t c = col0 + tx * 4 + j;
      if (c < ldo) out[r * ldo + c] = (c < m) ? (w ? val[i][j] * w[c] : val[i][j]) : 0.0;   // w == nullptr: Q = g
    }
  }
}

// ---- predictor gradient, composite programs of stationary leaves (Add / Mul / Pow, e.g. the time-sensitive
// product kernel):  grad_i = sum_l sum_j w_j (dP/dk_l)_ij g_l,ij (x_i - c_j)|dims_l.  One covariance-tile pass
// writes Q_l = w_j (dP/dk_l) g_l for every leaf l (the leaf dot products stay in registers, the adjoints come
// from the forward-mode evaluation of the program per element), then one GEMM T_l = Q_l [C|dims_l, 1] per leaf.
__global__ __launch_bounds__(256) void k_grad_coeff_multi(DevCov cov, const double* __restrict__ x, int64_t n,
                                                          const double* __restrict__ y, int64_t m, int d,
                                                          const double* __restrict__ xx, int64_t xx_stride,
                                                          const double* __restrict__ yy,
                                                          const double* __restrict__ w, double* __restrict__ out,
                                                          int64_t ldo, int64_t leaf_stride, int64_t tiles_n) {
  __shared__ double xs[DK][TM + PADT];
  __shared__ double ys[DK][TN + PADT];
  const int64_t bid = blockIdx.x;
  const int64_t row0 = (bid / tiles_n) * TM, col0 = (bid % tiles_n) * TN;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  double acc[MLN_MAX_LEAVES][4][4], xr[MLN_MAX_LEAVES][4], yr[MLN_MAX_LEAVES][4];
#pragma unroll
  for (int l = 0; l < MLN_MAX_LEAVES; ++l) {
    if (l >= cov.n_leaves) continue;            // uniform over the workgroup
    leaf_dot(cov, cov.leaves[l], x, n, y, m, d, row0, col0, xs, ys, acc[l]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t r = row0 + ty * 4 + i;
      xr[l][i] = (r < n) ? xx[(int64_t)l * xx_stride + r] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t c = col0 + tx * 4 + j;
      yr[l][j] = (c < m) ? yy[(int64_t)l * m + c] : 0.0;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t r = row0 + ty * 4 + i;
    if (r >= n) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t c = col0 + tx * 4 + j;
      if (c >= ldo) continue;
      double kv[MLN_MAX_LEAVES], gf[MLN_MAX_LEAVES], a[MLN_MAX_LEAVES];
#pragma unroll
      for (int l = 0; l < MLN_MAX_LEAVES; ++l) {
        kv[l] = 0.0; gf[l] = 0.0;
        if (l >= cov.n_leaves) continue;
        kv[l] = leaf_value(cov.leaves[l], xr[l][i], yr[l][j], acc[l][i][j]);
        gf[l] = leaf_grad_coeff(cov.leaves[l], xr[l][i], yr[l][j], acc[l][i][j]);
      }
      program_adjoints(cov, kv, a);
      const double wc = (c < m) ? (w ? w[c] : 1.0) : 0.0;   // w == nullptr: Q_l = (dP/dk_l) g_l (1.0 * v is v exactly)
#pragma unroll
      for (int l = 0; l < MLN_MAX_LEAVES; ++l)
        if (l < cov.n_leaves) out[(int64_t)l * leaf_stride + r * ldo + c] = wc * a[l] * gf[l];
    }
  }
}

// The centre operand of leaf l's GEMM, pb outputs side by side (W == nullptr: weight 1, the weights are in Q then):
//   Z_l[j][q (nd_l + 1) + k] = W[j][q0 + q] c_j[dims_l[k]] (k < nd_l),  W[j][q0 + q] (k == nd_l),  zero up to ldz
__global__ void k_grad_weighted_centres(DevCov cov, int leaf, const double* __restrict__ c, int64_t m, int d,
                                        const double* __restrict__ W, int64_t p, int64_t q0, int64_t pb,
                                        double* __restrict__ Z, int64_t ldz) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= m * ldz) return;
  const DevLeaf lf = cov.leaves[leaf];
  const int64_t j = idx / ldz, col = idx % ldz, nd1 = lf.ndims + 1;
  const int64_t q = col / nd1;
  const int k = (int)(col % nd1);
  double v = 0.0;
  if (q < pb) {
    const double ck = (k < lf.ndims) ? c[j * d + cov.dims[lf.dims_off + k]] : 1.0;
    v = W ? W[j * p + q0 + q] * ck : ck;
  }
  Z[idx] = v;
}

// out[i][q0 + q][dims_l[k]] += x_i[dims_l[k]] T_i,q(nd+1)+nd - T_i,q(nd+1)+k   (one thread per (i, q, k); out is rows x p x d,
// zeroed by the launcher; leaves and output blocks run one after the other on the stream)
__global__ void k_grad_combine_outputs(DevCov cov, int leaf, const double* __restrict__ T, int64_t ldt,
                                       const double* __restrict__ x, int64_t rows, int d, int64_t p, int64_t q0,
                                       int64_t pb, double* __restrict__ out) {
  const DevLeaf lf = cov.leaves[leaf];
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * pb * lf.ndims) return;
  const int k = (int)(idx % lf.ndims);
  const int64_t q = (idx / lf.ndims) % pb, i = idx / (lf.ndims * pb);
  const int dim = cov.dims[lf.dims_off + k];
  const double* __restrict__ Ti = T + i * ldt + q * (lf.ndims + 1);
  out[(i * p + q0 + q) * d + dim] += x[i * d + dim] * Ti[lf.ndims] - Ti[k];
}

// ---- predictor Hessian (base_predictor.py:507-521: jacfwd(jacrev(mean))) --------------------------------------
// With leaf gradients  grad k_l = gam_l (sig_l x - c)|dims_l  (stationary: gam = g, sig = 1; Linear: gam = -1/ls,
// sig = 0) and leaf Hessians  g_l I|dims_l + h_l (x - c)(x - c)^T|dims_l  (stationary only):
//   H_i = sum_j w_j [ sum_l a_l g_l I_l + sum_l (a_l h_l + a_ll gam_l^2) dl dl^T
//                     + sum_{l<l'} a_ll' gam_l gam_l' (dl dl'^T + dl' dl^T) ],   a_l = dP/dk_l, a_ll' = d2P/dk_l dk_l'
// One covariance-tile pass writes the coefficient matrices (Qd_l and one Qp per leaf pair); every pair then is
// ONE GEMM against [vec(c_l c_l'^T) | c_l | c_l' | 1] and an expansion of (sig x - c)(sig' x - c)^T.

__host__ __device__ inline int hess_pair_slot(int L, int l, int lp) {   // l <= lp: slots after the L diagonal ones
  return L + l * L - (l * (l - 1)) / 2 + (lp - l);
}

__global__ __launch_bounds__(256) void k_hess_coeff(DevCov cov, const double* __restrict__ x, int64_t n,
                                                    const double* __restrict__ y, int64_t m, int d,
                                                    const double* __restrict__ xx, int64_t xx_stride,
                                                    const double* __restrict__ yy,
                                                    const double* __restrict__ w, double* __restrict__ out,
                                                    int64_t ldo, int64_t slot_stride, int64_t tiles_n) {
  __shared__ double xs[DK][TM + PADT];
  __shared__ double ys[DK][TN + PADT];
  const int64_t bid = blockIdx.x;
  const int64_t row0 = (bid / tiles_n) * TM, col0 = (bid % tiles_n) * TN;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int L = cov.n_leaves;
  double acc[MLN_MAX_LEAVES][4][4], xr[MLN_MAX_LEAVES][4], yr[MLN_MAX_LEAVES][4];
#pragma unroll
  for (int l = 0; l < MLN_MAX_LEAVES; ++l) {
    if (l >= L) continue;
    leaf_dot(cov, cov.leaves[l], x, n, y, m, d, row0, col0, xs, ys, acc[l]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t r = row0 + ty * 4 + i;
      xr[l][i] = (r < n) ? xx[(int64_t)l * xx_stride + r] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t c = col0 + tx * 4 + j;
      yr[l][j] = (c < m) ? yy[(int64_t)l * m + c] : 0.0;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t r = row0 + ty * 4 + i;
    if (r >= n) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t c = col0 + tx * 4 + j;
      if (c >= ldo) continue;
      double kv[MLN_MAX_LEAVES], gam[MLN_MAX_LEAVES], gd[MLN_MAX_LEAVES], hc[MLN_MAX_LEAVES];
      double a1[MLN_MAX_LEAVES], a2[MLN_MAX_LEAVES][MLN_MAX_LEAVES];
#pragma unroll
      for (int l = 0; l < MLN_MAX_LEAVES; ++l) {
        kv[l] = 0.0; gam[l] = 0.0; gd[l] = 0.0; hc[l] = 0.0;
        if (l >= L) continue;
        const DevLeaf lf = cov.leaves[l];
        kv[l] = leaf_value(lf, xr[l][i], yr[l][j], acc[l][i][j]);
        if (lf.kind == MLN_K_LINEAR) { gam[l] = -lf.alpha_inv_ls[1]; continue; }
        gam[l] = gd[l] = leaf_grad_coeff(lf, xr[l][i], yr[l][j], acc[l][i][j]);
        hc[l] = leaf_hess_coeff(lf, xr[l][i], yr[l][j], acc[l][i][j]);
      }
      program_second(cov, kv, a1, a2);
      const double wc = (c < m) ? (w ? w[c] : 1.0) : 0.0;   // w == nullptr: the coefficients alone (1.0 * v is v exactly)
      const int64_t at = r * ldo + c;
#pragma unroll
      for (int l = 0; l < MLN_MAX_LEAVES; ++l) {
        if (l >= L) continue;
        out[(int64_t)l * slot_stride + at] = wc * a1[l] * gd[l];
#pragma unroll
        for (int lp = l; lp < MLN_MAX_LEAVES; ++lp) {
          if (lp >= L) continue;
          const double v = (lp == l) ? a1[l] * hc[l] + a2[l][l] * gam[l] * gam[l] : a2[l][lp] * gam[l] * gam[lp];
          out[(int64_t)hess_pair_slot(L, l, lp) * slot_stride + at] = wc * v;
        }
      }
    }
  }
}

// H_i[dim][dim] += sum_j Qd[i][j] for the dims of one stationary leaf: the diagonal term when the weights are in Qd
__global__ __launch_bounds__(256) void k_hess_diag(DevCov cov, int l, const double* __restrict__ Qd, int64_t ldq,
                                                   int64_t m, int64_t rows, int d, double* __restrict__ H) {
  __shared__ double red[256];
  const int64_t i = blockIdx.x;
  if (i >= rows) return;
  double s = 0.0;
  for (int64_t j = threadIdx.x; j < m; j += 256) s += Qd[i * ldq + j];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  const DevLeaf lf = cov.leaves[l];
  if (lf.kind == MLN_K_LINEAR) return;
  for (int k = threadIdx.x; k < lf.ndims; k += 256) {
    const int dim = cov.dims[lf.dims_off + k];
    H[i * (int64_t)d * d + (int64_t)dim * d + dim] += red[0];
  }
}

// The centre operand of a leaf pair's GEMM, pb outputs side by side, ncol = na nb + na + nb + 1 columns each (W == nullptr:
// weight 1, the weights are in the coefficient matrices then):
//   Z[j][q ncol + k] = W[j][q0 + q] [ c_j[dl[a]] c_j[dlp[b]] (k = a nb + b) | c_j[dl[a]] | c_j[dlp[b]] | 1 ], zero up to ldz
__global__ void k_hess_weighted_centres(DevCov cov, int l, int lp, const double* __restrict__ c, int64_t m, int d,
                                        const double* __restrict__ W, int64_t p, int64_t q0, int64_t pb,
                                        double* __restrict__ Z, int64_t ldz) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= m * ldz) return;
  const DevLeaf la = cov.leaves[l], lb = cov.leaves[lp];
  const int na = la.ndims, nb = lb.ndims, ncol = na * nb + na + nb + 1;
  const int64_t j = idx / ldz, col = idx % ldz, q = col / ncol;
  const int k = (int)(col % ncol);
  double v = 0.0;
  if (q < pb) {
    const double* cj = c + j * d;
    double ck = 1.0;
    if (k < na * nb) ck = cj[cov.dims[la.dims_off + k / nb]] * cj[cov.dims[lb.dims_off + k % nb]];
    else if (k < na * nb + na) ck = cj[cov.dims[la.dims_off + (k - na * nb)]];
    else if (k < na * nb + na + nb) ck = cj[cov.dims[lb.dims_off + (k - na * nb - na)]];
    v = W ? W[j * p + q0 + q] * ck : ck;
  }
  Z[idx] = v;
}

// Z[j][q] = W[j][q0 + q] (q < pb), zero up to ldz: the operand of the diagonal term's GEMM
__global__ void k_hess_weight_block(const double* __restrict__ W, int64_t m, int64_t p, int64_t q0, int64_t pb,
                                    double* __restrict__ Z, int64_t ldz) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= m * ldz) return;
  const int64_t j = idx / ldz, q = idx % ldz;
  Z[idx] = (q < pb) ? W[j * p + q0 + q] : 0.0;
}

// H is rows x ph x d x d, output q of the block goes to H[i][qoff + q]; T holds the block's pb outputs side by side (ncol
// columns each).  H[i][qoff + q][dl[a]][dlp[b]] (transpose = 0) or [dlp[b]][dl[a]] (transpose = 1)
//   += sig sig' s x_a x_b - sig x_a (Q c')_b - sig' (Q c)_a x_b + (Q c c'^T)_ab
__global__ void k_hess_combine_outputs(DevCov cov, int l, int lp, int transpose, const double* __restrict__ T, int64_t ldt,
                                       const double* __restrict__ x, int64_t rows, int d, int64_t ph, int64_t qoff,
                                       int64_t pb, double* __restrict__ H) {
  const DevLeaf la = cov.leaves[l], lb = cov.leaves[lp];
  const int na = la.ndims, nb = lb.ndims;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * pb * na * nb) return;
  const int ab = (int)(idx % (na * nb)), a = ab / nb, b = ab % nb;
  const int64_t q = (idx / (na * nb)) % pb, i = idx / ((int64_t)na * nb * pb);
  const int da = cov.dims[la.dims_off + a], db = cov.dims[lb.dims_off + b];
  const double sa = (la.kind == MLN_K_LINEAR) ? 0.0 : 1.0, sb = (lb.kind == MLN_K_LINEAR) ? 0.0 : 1.0;
  const double* Ti = T + i * ldt + q * (na * nb + na + nb + 1);
  const double xa = x[i * d + da], xb = x[i * d + db];
  const double val = sa * sb * Ti[na * nb + na + nb] * xa * xb - sa * xa * Ti[na * nb + na + b]
                     - sb * Ti[na * nb + a] * xb + Ti[ab];
  double* Hi = H + (i * ph + qoff + q) * (int64_t)d * d;
  if (transpose) Hi[db * d + da] += val; else Hi[da * d + db] += val;
}

// H[i][qoff + q][dim][dim] += Td[i][q] for the dims of one stationary leaf (Td = Qd_l W_block: k_hess_diag's row sum as a GEMM)
__global__ void k_hess_diag_outputs(DevCov cov, int l, const double* __restrict__ Td, int64_t ldt, int64_t rows, int d,
                                    int64_t ph, int64_t qoff, int64_t pb, double* __restrict__ H) {
  const DevLeaf lf = cov.leaves[l];
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * pb * lf.ndims) return;
  const int k = (int)(idx % lf.ndims);
  const int64_t q = (idx / lf.ndims) % pb, i = idx / ((int64_t)lf.ndims * pb);
  const int dim = cov.dims[lf.dims_off + k];
  H[(i * ph + qoff + q) * (int64_t)d * d + (int64_t)dim * d + dim] += Td[i * ldt + q];
}

int64_t pad16(int64_t v) { return ((v + 15) / 16) * 16; }

// a positive integer of at most `cap` from the environment, `dflt` without one (read at every call: the tests flip it)
int64_t env_positive(const char* name, int64_t dflt, int64_t cap) {
  const char* e = std::getenv(name);
  const long long v = e ? std::atoll(e) : 0;
  return (v >= 1 && v <= cap) ? v : dflt;
}

// outputs per block: as many as fit `cols` columns of the GEMM at `width` columns each, at least one, at most p
int64_t outputs_per_block(int64_t cols, int64_t width, int64_t p) {
  const int64_t pb = cols / width;
  return pb < 1 ? 1 : (pb > p ? p : pb);
}

// columns one output takes in the widest centre operand: nd_l + 1 (gradient), na nb + na + nb + 1 (Hessian)
int64_t grad_width(const DevCov& cov) {
  int64_t w = 1;
  for (int l = 0; l < cov.n_leaves; ++l) w = cov.leaves[l].ndims + 1 > w ? cov.leaves[l].ndims + 1 : w;
  return w;
}
int64_t hess_width(const DevCov& cov) {
  int64_t w = 1;
  for (int l = 0; l < cov.n_leaves; ++l)
    for (int lp = l; lp < cov.n_leaves; ++lp) {
      const int64_t na = cov.leaves[l].ndims, nb = cov.leaves[lp].ndims, ncol = na * nb + na + nb + 1;
      if (ncol > w) w = ncol;
    }
  return w;
}

GemmArgs plain_gemm(const double* A, int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc, int64_t M, int64_t N,
                    int64_t K) {
  GemmArgs g{};
  g.A = A; g.lda = lda; g.ta = 0; g.B = B; g.ldb = ldb; g.tb = 0; g.C = C; g.ldc = ldc;
  g.M = M; g.N = N; g.K = K; g.alpha = 1.0; g.beta = 0.0; g.split_k = 1;
  return g;
}

// The gradient of p outputs at every row of x, stationary leaves only (single leaf or composite program): out is n x p x d.
//   wq != nullptr (then W == nullptr, p == 1): the weights go into Q, Q_l = w_j (dP/dk_l) g_l, against the bare centres
//   W  != nullptr (m x p row-major):           Q_l = (dP/dk_l) g_l once per row chunk, whatever p is; the weights go into
//                                              the centre operand, pb <= pb_max outputs side by side
//   per row chunk (at most `chunk` rows):      one covariance-tile pass, k_grad_coeff for one bare leaf, else one matrix per leaf
//   per output block [q0, q0 + pb) and leaf:   T = Q_l Z_l, one GEMM of pb (nd_l + 1) columns;  out[:, q0 + q, dims_l] += x T_nd - T_k
int gradient_pass(mln_ctx* ctx, const DevCov& cov, const double* x, int64_t n, const double* c, int64_t m, int d,
                  const double* wq, const double* W, int64_t p, int64_t chunk, int64_t pb_max, double* out) {
  if (!wq == !W || (wq && p != 1)) {
    mln_set_error(ctx, "gradient_pass: weights in Q go with one output and no W");
    return MLN_ERR_UNSUPPORTED;
  }
  const int L = cov.n_leaves;
  const int64_t ldq = pad16(m), ldz = pad16(pb_max * grad_width(cov));
  if (chunk > n) chunk = n;
  const bool single = cov.n_toks == 1;
  const bool z_fixed = wq && L == 1;          // one leaf, bare centres: the operand is the same for every row chunk
  double* norms = nullptr;
  DevBuf<double> Q, T, Z;
  MLN_TRY(mln_scratch(ctx, sizeof(double) * (size_t)L * (size_t)(n + m), (void**)&norms));
  double* xx = norms;                        // [L][n]
  double* yy = norms + (size_t)L * n;        // [L][m]
  MLN_TRY(launch_leaf_sqnorms(ctx, cov, x, n, d, xx));
  MLN_TRY(launch_leaf_sqnorms(ctx, cov, c, m, d, yy));
  const int64_t leaf_stride = chunk * ldq;
  MLN_TRY(Q.alloc(ctx, (size_t)L * leaf_stride, "Q"));
  MLN_TRY(T.alloc(ctx, (size_t)chunk * ldz, "T"));
  MLN_TRY(Z.alloc(ctx, (size_t)m * ldz, "Z"));
  MLN_HIP(ctx, hipMemsetAsync(out, 0, sizeof(double) * (size_t)n * (size_t)p * d, ctx->stream));
  int rc = MLN_OK;
  const int64_t tiles_n = (ldq + TN - 1) / TN;
  for (int64_t r0 = 0; r0 < n && rc == MLN_OK; r0 += chunk) {
    const int64_t rows = (n - r0 < chunk) ? (n - r0) : chunk;
    const int64_t nblk = tiles_n * ((rows + TM - 1) / TM);
    if (single)
      hipLaunchKernelGGL(k_grad_coeff, dim3((unsigned)nblk), dim3(256), 0, ctx->stream, cov, x + r0 * d, rows, c, m, d,
                         xx + r0, yy, wq, Q.get(), ldq, tiles_n);
    else
      hipLaunchKernelGGL(k_grad_coeff_multi, dim3((unsigned)nblk), dim3(256), 0, ctx->stream, cov, x + r0 * d, rows, c, m,
                         d, xx + r0, n, yy, wq, Q.get(), ldq, leaf_stride, tiles_n);
    for (int64_t q0 = 0; q0 < p && rc == MLN_OK; q0 += pb_max) {
      const int64_t pb = (p - q0 < pb_max) ? (p - q0) : pb_max;
      for (int l = 0; l < L && rc == MLN_OK; ++l) {
        const int nd = cov.leaves[l].ndims;
        if (nd == 0) continue;
        if (!z_fixed || r0 == 0)
          hipLaunchKernelGGL(k_grad_weighted_centres, dim3((unsigned)((m * ldz + 255) / 256)), dim3(256), 0, ctx->stream,
                             cov, l, c, m, d, W, p, q0, pb, Z.get(), ldz);
        rc = launch_dgemm(ctx, plain_gemm(Q + (size_t)l * leaf_stride, ldq, Z, ldz, T, ldz, rows, pb * (nd + 1), m));
        if (rc != MLN_OK) break;
        hipLaunchKernelGGL(k_grad_combine_outputs, dim3((unsigned)((rows * pb * nd + 255) / 256)), dim3(256), 0,
                           ctx->stream, cov, l, T.get(), ldz, x + r0 * d, rows, d, p, q0, pb, out + r0 * p * d);
      }
    }
  }
  hipError_t e = hipGetLastError();
  (void)hipStreamSynchronize(ctx->stream);
  if (rc == MLN_OK && e != hipSuccess) rc = mln_hip_fail(ctx, e, "predict_gradient", __FILE__, __LINE__);
  return rc;
}

// The Hessian of p outputs at every row of x (see k_hess_coeff), any program (a Linear factor is sig = 0 inside the same GEMM
// formulation).  out != nullptr: the Hessians, n x p x d x d; out == nullptr: every (row chunk, output block) of Hessians is
// built in scratch and factored there, only sign / logabs (n x p) of the leading lead x lead blocks are written.  Both are
// this one loop: the fused entry factors the bits the other returns.
//   wq != nullptr (then W == nullptr, p == 1): the weights go into the coefficient matrices; the diagonal term is their row
//                                              sum (k_hess_diag)
//   W  != nullptr (m x p row-major):           weight-less coefficients once per row chunk, whatever p is; the weights go into
//                                              the centre operands, pb <= pb_max outputs side by side; the diagonal term is
//                                              the GEMM Td = Qd_l W[:, q0 .. q0 + pb)  (the two forms sum in different orders)
//   per output block, per leaf pair:           T = Qp_ll' Z_ll', one GEMM of pb ncol_ll' columns, expanded by k_hess_combine_outputs
int hessian_pass(mln_ctx* ctx, const DevCov& cov, const double* x, int64_t n, const double* c, int64_t m, int d,
                 const double* wq, const double* W, int64_t p, int64_t chunk, int64_t pb_max, double* out, int lead,
                 double* sign, double* logabs) {
  if (!wq == !W || (wq && (p != 1 || !out))) {     // (k_hess_diag writes H as rows x d x d)
    mln_set_error(ctx, "hessian_pass: weights in Q go with one output, no W and a result array");
    return MLN_ERR_UNSUPPORTED;
  }
  const int L = cov.n_leaves;
  const int n_slots = L + (L * (L + 1)) / 2;
  const int64_t ldq = pad16(m), ldz = pad16(pb_max * hess_width(cov));
  const int64_t dd = (int64_t)d * d;
  if (chunk > n) chunk = n;
  const bool z_fixed = wq && L == 1;          // one leaf pair, bare centres, k_hess_diag needs no operand: Z never changes
  double* norms = nullptr;
  DevBuf<double> Q, T, Z, Hs;
  MLN_TRY(mln_scratch(ctx, sizeof(double) * (size_t)L * (size_t)(n + m), (void**)&norms));
  double* xx = norms;
  double* yy = norms + (size_t)L * n;
  MLN_TRY(launch_leaf_sqnorms(ctx, cov, x, n, d, xx));
  MLN_TRY(launch_leaf_sqnorms(ctx, cov, c, m, d, yy));
  const int64_t slot_stride = chunk * ldq;
  MLN_TRY(Q.alloc(ctx, (size_t)n_slots * slot_stride, "Q"));
  MLN_TRY(T.alloc(ctx, (size_t)chunk * ldz, "T"));
  MLN_TRY(Z.alloc(ctx, (size_t)m * ldz, "Z"));
  if (out) MLN_HIP(ctx, hipMemsetAsync(out, 0, sizeof(double) * (size_t)n * (size_t)p * dd, ctx->stream));
  else MLN_TRY(Hs.alloc(ctx, (size_t)chunk * pb_max * dd, "Hs"));
  int rc = MLN_OK;
  const int64_t tiles_n = (ldq + TN - 1) / TN;
  const unsigned zblocks = (unsigned)((m * ldz + 255) / 256);
  for (int64_t r0 = 0; r0 < n && rc == MLN_OK; r0 += chunk) {
    const int64_t rows = (n - r0 < chunk) ? (n - r0) : chunk;
    const int64_t nblk = tiles_n * ((rows + TM - 1) / TM);
    const double* xc = x + r0 * d;
    hipLaunchKernelGGL(k_hess_coeff, dim3((unsigned)nblk), dim3(256), 0, ctx->stream, cov, xc, rows, c, m, d, xx + r0, n, yy,
                       wq, Q.get(), ldq, slot_stride, tiles_n);
    for (int64_t q0 = 0; q0 < p && rc == MLN_OK; q0 += pb_max) {
      const int64_t pb = (p - q0 < pb_max) ? (p - q0) : pb_max;
      double* H = out ? out + r0 * p * dd : Hs.get();
      const int64_t ph = out ? p : pb, qoff = out ? q0 : 0;
      if (!out) {
        const hipError_t em = hipMemsetAsync(H, 0, sizeof(double) * (size_t)(rows * pb * dd), ctx->stream);
        if (em != hipSuccess) { rc = mln_hip_fail(ctx, em, "predict_hessian_logdet", __FILE__, __LINE__); break; }
      }
      for (int l = 0; l < L && rc == MLN_OK; ++l) {
        const int na = cov.leaves[l].ndims;
        if (na == 0) continue;
        if (cov.leaves[l].kind != MLN_K_LINEAR && wq) {
          hipLaunchKernelGGL(k_hess_diag, dim3((unsigned)rows), dim3(256), 0, ctx->stream, cov, l,
                             Q + (size_t)l * slot_stride, ldq, m, rows, d, H);
        } else if (cov.leaves[l].kind != MLN_K_LINEAR) {
          hipLaunchKernelGGL(k_hess_weight_block, dim3(zblocks), dim3(256), 0, ctx->stream, W, m, p, q0, pb, Z.get(), ldz);
          rc = launch_dgemm(ctx, plain_gemm(Q + (size_t)l * slot_stride, ldq, Z, ldz, T, ldz, rows, pb, m));
          if (rc != MLN_OK) break;
          hipLaunchKernelGGL(k_hess_diag_outputs, dim3((unsigned)((rows * pb * na + 255) / 256)), dim3(256), 0, ctx->stream,
                             cov, l, T.get(), ldz, rows, d, ph, qoff, pb, H);
        }
        for (int lp = l; lp < L && rc == MLN_OK; ++lp) {
          const int nb = cov.leaves[lp].ndims;
          if (nb == 0) continue;
          if (!z_fixed || r0 == 0)
            hipLaunchKernelGGL(k_hess_weighted_centres, dim3(zblocks), dim3(256), 0, ctx->stream, cov, l, lp, c, m, d, W, p,
                               q0, pb, Z.get(), ldz);
          rc = launch_dgemm(ctx, plain_gemm(Q + (size_t)hess_pair_slot(L, l, lp) * slot_stride, ldq, Z, ldz, T, ldz, rows,
                                            pb * ((int64_t)na * nb + na + nb + 1), m));
          if (rc != MLN_OK) break;
          const unsigned nb_ = (unsigned)((rows * pb * na * nb + 255) / 256);
          hipLaunchKernelGGL(k_hess_combine_outputs, dim3(nb_), dim3(256), 0, ctx->stream, cov, l, lp, 0, T.get(), ldz, xc,
                             rows, d, ph, qoff, pb, H);
          if (lp != l)
            hipLaunchKernelGGL(k_hess_combine_outputs, dim3(nb_), dim3(256), 0, ctx->stream, cov, l, lp, 1, T.get(), ldz, xc,
                               rows, d, ph, qoff, pb, H);
        }
      }
      if (!out && rc == MLN_OK)
        rc = launch_slogdet_batched(ctx, H, rows * pb, d, dd, lead, sign + r0 * p, logabs + r0 * p, pb, p, q0);
    }
  }
  hipError_t e = hipGetLastError();
  (void)hipStreamSynchronize(ctx->stream);
  if (rc == MLN_OK && e != hipSuccess) rc = mln_hip_fail(ctx, e, "predict_hessian", __FILE__, __LINE__);
  return rc;
}

// rows per chunk of launch_predict_hessian before it is clamped to n: <= 2 GiB of coefficient matrices per chunk
int64_t hess_single_chunk(int L, int64_t m) {
  int64_t chunk = ((int64_t)1 << 28) / (pad16(m) * (L + (L * (L + 1)) / 2));
  if (chunk > 16384) chunk = 16384;
  if (chunk < 64) chunk = 64;
  return chunk;
}

// ---- p outputs (W m x p row-major) --------------------------------------------------------------------------------------------
// At most GRAD_MULTI_COLS / HESS_MULTI_COLS columns per GEMM (MELLON_AMD_GRAD_COLS / MELLON_AMD_HESS_COLS override them, read at
// every call).  Rows per chunk: a multiple of 64, never below 64, at most the single-output launcher's cap (32768 / 16384), and
// Q plus T -- and for the Hessian one output block of Hessians, pb d^2 per row, which only the fused entry allocates but both
// count, so that both walk the same row chunks -- within *_MULTI_SCRATCH doubles.
constexpr int64_t GRAD_MULTI_COLS = 512;
constexpr int64_t GRAD_MULTI_SCRATCH = (int64_t)1 << 27;   // 1 GiB of doubles for Q and T together
constexpr int64_t HESS_MULTI_COLS = 4096;
constexpr int64_t HESS_MULTI_SCRATCH = (int64_t)1 << 28;   // 2 GiB of doubles
constexpr int64_t MULTI_MIN_PAIRS = (int64_t)1 << 16;      // the threshold of the single-output GEMM routes

int64_t multi_chunk(int64_t scratch, int64_t doubles_per_row, int64_t cap) {
  int64_t chunk = (scratch / doubles_per_row / 64) * 64;
  if (chunk > cap) chunk = cap;
  return chunk < 64 ? 64 : chunk;
}

int gradient_batched(mln_ctx* ctx, const DevCov& cov, const double* x, int64_t n, const double* c, int64_t m, int d,
                     const double* W, int64_t p, double* out) {
  const int64_t width = grad_width(cov);
  const int64_t pb_max = outputs_per_block(env_positive("MELLON_AMD_GRAD_COLS", GRAD_MULTI_COLS, 4096), width, p);
  const int64_t chunk = multi_chunk(GRAD_MULTI_SCRATCH, (int64_t)cov.n_leaves * pad16(m) + pad16(pb_max * width), 32768);
  return gradient_pass(ctx, cov, x, n, c, m, d, nullptr, W, p, chunk, pb_max, out);
}

int hessian_batched(mln_ctx* ctx, const DevCov& cov, const double* x, int64_t n, const double* c, int64_t m, int d,
                    const double* W, int64_t p, double* out, int lead, double* sign, double* logabs) {
  const int L = cov.n_leaves;
  const int64_t width = hess_width(cov);
  const int64_t pb_max = outputs_per_block(env_positive("MELLON_AMD_HESS_COLS", HESS_MULTI_COLS, 65536), width, p);
  const int64_t per_row = (int64_t)(L + (L * (L + 1)) / 2) * pad16(m) + pad16(pb_max * width) + pb_max * d * d;
  return hessian_pass(ctx, cov, x, n, c, m, d, nullptr, W, p, multi_chunk(HESS_MULTI_SCRATCH, per_row, 16384), pb_max, out,
                      lead, sign, logabs);
}

// Column by column through a single-output launcher (gathered weights, scattered result): its bits.  out is n x p x width.
using SingleOutput = int (*)(mln_ctx*, const DevCov&, const double*, int64_t, const double*, int64_t, int, const double*, double*);
int per_column(mln_ctx* ctx, SingleOutput single, const DevCov& cov, const double* x, int64_t n, const double* c, int64_t m,
               int d, const double* W, int64_t p, int64_t width, double* out) {
  DevBuf<double> wq, oq;
  if (m > 0) MLN_TRY(wq.alloc(ctx, (size_t)m, "wq"));
  MLN_TRY(oq.alloc(ctx, (size_t)n * width, "oq"));
  for (int64_t q = 0; q < p; ++q) {
    MLN_TRY(launch_copy_block(ctx, W + q, p, wq.get(), 1, m, 1));
    MLN_TRY(single(ctx, cov, x, n, c, m, d, wq.get(), oq.get()));
    MLN_TRY(launch_copy_block(ctx, oq.get(), width, out + q * width, p * width, n, width));
  }
  MLN_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MLN_OK;
}

bool all_stationary(const DevCov& cov) {
  bool stationary = cov.n_leaves >= 1;
  for (int l = 0; l < cov.n_leaves; ++l) stationary = stationary && cov.leaves[l].kind != MLN_K_LINEAR;
  return stationary;
}

}  // namespace

// One output, weights in Q, row chunks of 32768: the GEMM route of launch_predict_gradient (cov_grad.hip) for programs whose
// leaves are all stationary.
int launch_predict_gradient_gemm(mln_ctx* ctx, const DevCov& cov, const double* x, int64_t n, const double* c,
                                 int64_t m, int d, const double* w, double* out) {
  if (n == 0) return MLN_OK;
  return gradient_pass(ctx, cov, x, n, c, m, d, w, nullptr, 1, 32768, 1, out);
}

// Gradient of a p-output predictive mean: out[i][q][:] = sum_j W[j][q] d cov(x_i, c_j) / d x_i   (out: n x p x d).
//   p == 1                                   launch_predict_gradient itself
//   stationary leaves only, n m >= 2^16      gradient_batched: the covariance epilogue once per pair
//   anything else                            launch_predict_gradient per column
int launch_predict_gradient_multi(mln_ctx* ctx, const DevCov& cov, const double* x, int64_t n, const double* c, int64_t m,
                                  int d, const double* W, int64_t p, double* out) {
  if (n == 0 || p == 0) return MLN_OK;
  if (p == 1) return launch_predict_gradient(ctx, cov, x, n, c, m, d, W, out);
  if (all_stationary(cov) && n * m >= MULTI_MIN_PAIRS) return gradient_batched(ctx, cov, x, n, c, m, d, W, p, out);
  return per_column(ctx, launch_predict_gradient, cov, x, n, c, m, d, W, p, d, out);
}

// Hessian of the predicted mean at every row of x, one output: out is n x d x d.
int launch_predict_hessian(mln_ctx* ctx, const DevCov& cov, const double* x, int64_t n, const double* c, int64_t m,
                           int d, const double* w, double* out) {
  if (n == 0) return MLN_OK;
  return hessian_pass(ctx, cov, x, n, c, m, d, w, nullptr, 1, hess_single_chunk(cov.n_leaves, m), 1, out, 0, nullptr, nullptr);
}

// Hessians of p outputs: out is n x p x d x d.
//   p == 1                     launch_predict_hessian itself
//   n m < 2^16                 launch_predict_hessian per column
//   anything else, any program hessian_batched
int launch_predict_hessian_multi(mln_ctx* ctx, const DevCov& cov, const double* x, int64_t n, const double* c, int64_t m,
                                 int d, const double* W, int64_t p, double* out) {
  if (n == 0 || p == 0) return MLN_OK;
  if (p == 1) return launch_predict_hessian(ctx, cov, x, n, c, m, d, W, out);
  if (n * m >= MULTI_MIN_PAIRS) return hessian_batched(ctx, cov, x, n, c, m, d, W, p, out, 0, nullptr, nullptr);
  return per_column(ctx, launch_predict_hessian, cov, x, n, c, m, d, W, p, (int64_t)d * d, out);
}

// sign / logabs (n x p) of the leading lead x lead block of every Hessian: only these reach the caller.  The batched route
// factors each (row chunk, output block) in scratch; the single-output routes run on row blocks that are whole multiples of
// launch_predict_hessian's own chunk (the launches, hence the bits, of the unfused call), within HESS_MULTI_SCRATCH doubles
// of Hessians where one such chunk allows.
int launch_predict_hessian_logdet(mln_ctx* ctx, const DevCov& cov, const double* x, int64_t n, const double* c, int64_t m,
                                  int d, const double* W, int64_t p, int lead, double* sign, double* logabs) {
  if (n == 0 || p == 0) return MLN_OK;
  if (p > 1 && n * m >= MULTI_MIN_PAIRS) return hessian_batched(ctx, cov, x, n, c, m, d, W, p, nullptr, lead, sign, logabs);
  const int64_t dd = (int64_t)d * d, step = hess_single_chunk(cov.n_leaves, m);
  int64_t rb = (HESS_MULTI_SCRATCH / (p * dd)) / step * step;
  if (rb < step) rb = step;
  if (rb > n) rb = n;
  DevBuf<double> Hs;
  MLN_TRY(Hs.alloc(ctx, (size_t)rb * p * dd, "Hs"));
  for (int64_t r0 = 0; r0 < n; r0 += rb) {
    const int64_t rows = (n - r0 < rb) ? (n - r0) : rb;
    MLN_TRY(launch_predict_hessian_multi(ctx, cov, x + r0 * d, rows, c, m, d, W, p, Hs.get()));
    MLN_TRY(launch_slogdet_batched(ctx, Hs.get(), rows * p, d, dd, lead, sign + r0 * p, logabs + r0 * p, 1, 1, 0));
  }
  MLN_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MLN_OK;
}
