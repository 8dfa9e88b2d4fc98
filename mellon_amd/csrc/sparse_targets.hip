// FunctionEstimator targets kept sparse (CSR) from the caller's arrays to HBM: the landmark conditional needs
// C = L^T (y - mu) and nothing else of y, so y - mu is only ever formed as a panel of rows -- built from the CSR arrays by
// k_csr_panel, consumed by the fp64 GEMM, overwritten by the next panel.  No n x p array exists on the host or the device.
#include "api_internal.h"

#include <cinttypes>

// Bytes of one row panel of y - mu (mirrored as _lib.CSR_PANEL_BYTES).  Rows per panel = budget / (8 p), rounded down to
// a multiple of 64, at least 64.
static constexpr int64_t CSR_PANEL_BYTES = 64ll << 20;
static constexpr int CSR_WG_THREADS = 256;
static constexpr int64_t CSR_WG_ELEMS = 8192;    // elements of the panel one workgroup fills between two barriers

static int64_t csr_panel_rows(int64_t p) {
  int64_t rows = CSR_PANEL_BYTES / (8 * p);
  rows -= rows % 64;
  return rows < 64 ? 64 : rows;
}

// Panel R[0 : rows, 0 : p] (pitch p) = y[r0 : r0 + rows] - mu from the CSR arrays of y.  A workgroup owns whole rows,
// `rows_per_wg` adjacent ones at a time: it fills them with 0 - mu (16-byte stores over the one contiguous range they
// occupy), waits at the barrier, then overwrites the stored entries of the same rows with data - mu.  No element is touched
// by two workgroups, so there is nothing to order between them and nothing atomic.  Every store is guarded here as well
// (row < n, 0 <= j < p, 0 <= q < nnz): arrays the entry's validation would have refused still write nothing out of bounds.
__global__ __launch_bounds__(CSR_WG_THREADS) void k_csr_panel(const int64_t* __restrict__ indptr,
                                                               const int32_t* __restrict__ indices,
                                                               const double* __restrict__ data, int64_t nnz, int64_t n,
                                                               int64_t r0, int64_t rows, int64_t p, int64_t rows_per_wg,
                                                               double mu, double* __restrict__ R) {
  const double fill = 0.0 - mu;
  const int tid = (int)threadIdx.x;
  for (int64_t c = blockIdx.x; c * rows_per_wg < rows; c += gridDim.x) {      // (uniform per workgroup: the barrier is safe)
    const int64_t a = c * rows_per_wg;
    int64_t b = a + rows_per_wg;
    if (b > rows) b = rows;
    if (r0 + b > n) b = n - r0;
    if (b < a) b = a;
    double* base = R + a * p;
    const int64_t count = (b - a) * p;
    const int64_t head = (count > 0 && ((uintptr_t)base & 8)) ? 1 : 0;      // one element up to the 16-byte boundary
    const int64_t pairs = (count - head) / 2;
    double2* v = reinterpret_cast<double2*>(base + head);
    for (int64_t i = tid; i < pairs; i += CSR_WG_THREADS) v[i] = make_double2(fill, fill);
    if (tid == 0 && head) base[0] = fill;
    if (tid == 0 && head + 2 * pairs < count) base[count - 1] = fill;
    __syncthreads();
    // the stored entries: the workgroup's threads in 1, 2 or 4 groups, one row per group at a time
    const int64_t nrows = b - a;
    const int groups = nrows >= 3 ? 4 : (nrows == 2 ? 2 : 1), width = CSR_WG_THREADS / groups;
    const int group = tid / width, lane = tid % width;
    for (int64_t row = a + group; row < b; row += groups) {
      int64_t q0 = indptr[r0 + row], q1 = indptr[r0 + row + 1];
      if (q0 < 0) q0 = 0;
      if (q1 > nnz) q1 = nnz;
      for (int64_t q = q0 + lane; q < q1; q += width) {
        const int64_t j = indices[q];
        if (j >= 0 && j < p) R[row * p + j] = data[q] - mu;
      }
    }
  }
}

int csr_targets_product(mln_ctx* ctx, const double* L, int64_t ldl, int64_t m, int64_t n, int64_t p,
                        const CsrTargets& y, double mu, double alpha, double* C) {
  const size_t stride = (size_t)m * p;
  MLN_HIP(ctx, hipMemsetAsync(C, 0, sizeof(double) * stride, ctx->stream));
  if (n <= 0) return MLN_OK;
  int64_t panel = csr_panel_rows(p);
  if (panel > n) panel = n;
  // the k-split of the dense route, per panel
  int split = (int)(panel / 8192);
  if (split < 1) split = 1;
  if (split > 16) split = 16;
  DevBuf<int64_t> d_indptr;
  DevBuf<int32_t> d_indices;
  DevBuf<double> d_data, R, parts;
  MLN_TRY(d_indptr.alloc(ctx, (size_t)n + 1, "CSR indptr"));
  MLN_TRY(d_indices.alloc(ctx, (size_t)(y.nnz > 0 ? y.nnz : 1), "CSR indices"));
  MLN_TRY(d_data.alloc(ctx, (size_t)(y.nnz > 0 ? y.nnz : 1), "CSR data"));
  MLN_TRY(R.alloc(ctx, (size_t)panel * p, "CSR row panel"));
  MLN_TRY(parts.alloc(ctx, stride * split, "parts"));
  int rc = MLN_OK;
  auto chk = [&](hipError_t e) { if (e != hipSuccess && rc == MLN_OK) rc = mln_hip_fail(ctx, e, "csr_targets_product", __FILE__, __LINE__); };
  chk(hipMemcpyAsync(d_indptr, y.indptr, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, ctx->stream));
  if (y.nnz > 0) {
    chk(hipMemcpyAsync(d_indices, y.indices, sizeof(int32_t) * (size_t)y.nnz, hipMemcpyHostToDevice, ctx->stream));
    chk(hipMemcpyAsync(d_data, y.data, sizeof(double) * (size_t)y.nnz, hipMemcpyHostToDevice, ctx->stream));
  }
  int64_t rows_per_wg = CSR_WG_ELEMS / p;
  if (rows_per_wg < 1) rows_per_wg = 1;
  for (int64_t r0 = 0; r0 < n && rc == MLN_OK; r0 += panel) {
    const int64_t rows = (n - r0 < panel) ? n - r0 : panel;
    int64_t nwg = (rows + rows_per_wg - 1) / rows_per_wg;
    if (nwg > 4096) nwg = 4096;
    hipLaunchKernelGGL(k_csr_panel, dim3((unsigned)nwg), dim3(CSR_WG_THREADS), 0, ctx->stream, d_indptr.get(),
                       d_indices.get(), d_data.get(), y.nnz, n, r0, rows, p, rows_per_wg, mu, R.get());
    chk(hipGetLastError());
    GemmArgs g{};
    g.A = L + r0 * ldl; g.lda = ldl; g.B = R; g.ldb = p; g.C = parts; g.ldc = p;
    g.M = m; g.N = p; g.K = rows; g.alpha = alpha; g.beta = 0.0; g.ta = 1; g.tb = 0;
    g.split_k = split; g.c_split_stride = (int64_t)stride;
    if (rc == MLN_OK) rc = launch_dgemm(ctx, g);
    // C += the panel's partial products, in the order of the k-chunks: panels and chunks in a fixed order
    if (rc == MLN_OK) rc = launch_sum_partials(ctx, parts, split, (int64_t)stride, C, (int64_t)stride, r0 > 0 ? 1.0 : 0.0);
  }
  chk(hipStreamSynchronize(ctx->stream));
  return rc;
}

// One host pass over the arrays, before anything is launched.
static int csr_validate(mln_ctx* ctx, const int64_t* indptr, const int32_t* indices, const double* data, int64_t n,
                        int64_t p) {
  char msg[160];
  if (indptr[0] != 0) { mln_set_error(ctx, "CSR targets: indptr[0] must be 0"); return MLN_ERR_ARG; }
  for (int64_t i = 0; i < n; ++i) {
    const int64_t q0 = indptr[i], q1 = indptr[i + 1];
    if (q1 < q0) {
      snprintf(msg, sizeof msg, "CSR targets: indptr decreases at row %" PRId64, i);
      mln_set_error(ctx, msg);
      return MLN_ERR_ARG;
    }
    if (q1 > q0 && (!indices || !data)) return MLN_ERR_ARG;
    for (int64_t q = q0; q < q1; ++q) {
      const int64_t j = indices[q];
      if (j < 0 || j >= p || (q > q0 && j <= indices[q - 1])) {
        snprintf(msg, sizeof msg, "CSR targets: row %" PRId64 " has column index %" PRId64 " %s", i, j,
                 (j < 0 || j >= p) ? "outside [0, p)" : "not above the one before it (indices must be sorted, without duplicates)");
        mln_set_error(ctx, msg);
        return MLN_ERR_ARG;
      }
      if (!std::isfinite(data[q])) {
        snprintf(msg, sizeof msg, "CSR targets: row %" PRId64 " holds a non-finite value", i);
        mln_set_error(ctx, msg);
        return MLN_ERR_ARG;
      }
    }
  }
  return MLN_OK;
}

extern "C" int mln_sparse_solve_csr(mln_ctx* ctx, const mln_kernel_desc* cov, const double* x, int64_t n_local, int32_t d,
                                    const double* xu, int64_t m, const int64_t* indptr, const int32_t* indices,
                                    const double* data, int64_t p, double mu, const double* sigma, int32_t sigma_kind,
                                    double jitter, double* W, double* Lp_out, double* Cs_out) {
  if (!ctx || !indptr || !sigma || n_local < 0) return MLN_ERR_ARG;
  if (p < 1 || p > 0x7fffffffLL) { mln_set_error(ctx, "CSR targets: p must lie in [1, 2^31)"); return MLN_ERR_SHAPE; }
  if (sigma_kind != MLN_SIGMA_SCALAR && sigma_kind != MLN_SIGMA_PER_OUTPUT) {
    mln_set_error(ctx, "CSR targets take one sigma or one per output column (one sigma per cell is a model of a 1-D y)");
    return MLN_ERR_ARG;
  }
  if (is_device_ptr(indptr) || (indices && is_device_ptr(indices)) || (data && is_device_ptr(data))) {
    mln_set_error(ctx, "CSR targets: indptr, indices and data are host arrays");
    return MLN_ERR_ARG;
  }
  MLN_TRY(csr_validate(ctx, indptr, indices, data, n_local, p));
  const CsrTargets y{indptr, indices, data, indptr[n_local]};
  return sparse_solve_impl(ctx, cov, x, n_local, d, xu, m, nullptr, p, mu, sigma, sigma_kind, jitter, W, Lp_out, Cs_out, &y);
}
