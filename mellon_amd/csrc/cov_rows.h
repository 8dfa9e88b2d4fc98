// Shared pieces and launchers of the persistent-row covariance kernels (rows_pipeline.h; the 1-NN kernel shares the tile
// constants).
#pragma once
#include "mln_core.h"

typedef double v4d_t __attribute__((ext_vector_type(4)));

namespace covrows {
constexpr int TN = 64;    // centres per tile
constexpr int NNS = 65;   // LDS row stride (doubles), odd: the 16 lanes of one ds_read2_b64 group (li = 0..15, one k) land on 16 distinct bank pairs
}  // namespace covrows

// Persistent-row launchers (cov_rows.hip).  One stationary leaf over all d <= 64 contiguous columns:
int launch_kernel_matrix_rows_q(mln_ctx* ctx, const DevCov& cov, const double* x, int64_t n, const double* y, int64_t m,
                                int d, const double* xx, const double* yy, double* out, int64_t ldo, double add_diag,
                                float* out32, int q32);
int launch_predict_mean_rows(mln_ctx* ctx, const DevCov& cov, const double* x, int64_t n, const double* y, int64_t m,
                             int d, const double* xx, const double* yy, const double* w, double mu, double* out);
// The time-sensitive product kernel (state leaf x time leaf; xx0, yy0: the norms of the state columns):
bool predict_rows_prod_eligible(const DevCov& cov, int d);
int launch_kernel_matrix_rows_prod(mln_ctx* ctx, const DevCov& cov, const double* x, int64_t n, const double* y, int64_t m,
                                   int d, const double* xx0, const double* yy0, double* out, int64_t ldo, double add_diag,
                                   float* out32, int q32);
int launch_predict_mean_rows_prod(mln_ctx* ctx, const DevCov& cov, const double* x, int64_t n, const double* y, int64_t m,
                                  int d, const double* xx0, const double* yy0, const double* w, double mu, double* out);

// Their kernels.  The launchers are declared here and defined by explicit instantiation or specialisation in one
// translation unit per kind and family, so a unit missing from the build shows as an undefined launch_*_rows_kind<KIND, PROD>:
//   launch_kernel_matrix_rows_kind<KIND, false>   cov_rows_<kind>.hip           (cov_rows_impl.h, on rows_pipeline.h)
//   launch_kernel_matrix_rows_kind<KIND, true>    kernel_rows_prod_<kind>.hip   (kernel_rows_prod_impl.h, its own pipeline)
//   launch_predict_mean_rows_kind<KIND, false>    predict_rows_<kind>.hip       (predict_rows_impl.h, on rows_pipeline.h)
//   launch_predict_mean_rows_kind<KIND, true>     predict_rows_prod_<kind>.hip  (predict_rows_impl.h)
template <int KIND, bool PROD>
int launch_kernel_matrix_rows_kind(mln_ctx* ctx, const DevCov& cov, const double* x, int64_t n, const double* y, int64_t m,
                                   int d, const double* xx, const double* yy, double* out, int64_t ldo, double add_diag,
                                   float* out32, int q32);
template <int KIND, bool PROD>
int launch_predict_mean_rows_kind(mln_ctx* ctx, const DevCov& cov, const double* x, int64_t n, const double* y, int64_t m,
                                  int d, const double* xx, const double* yy, const double* w, double mu, double* out);
#define MLN_INSTANTIATE_KERNEL_MATRIX_ROWS(KIND, PROD)                                                            \
  template int launch_kernel_matrix_rows_kind<KIND, PROD>(mln_ctx*, const DevCov&, const double*, int64_t, const double*, \
                                                          int64_t, int, const double*, const double*, double*, int64_t,   \
                                                          double, float*, int);
#define MLN_INSTANTIATE_PREDICT_MEAN_ROWS(KIND, PROD)                                                            \
  template int launch_predict_mean_rows_kind<KIND, PROD>(mln_ctx*, const DevCov&, const double*, int64_t, const double*, \
                                                         int64_t, int, const double*, const double*, const double*,      \
                                                         double, double*);
