// Shared by the translation units behind the C ABI (api*.hip): the fit handle, the host/device pointer wrappers and the
// helpers that cross the file boundaries.  (Round 4: csrc/api.hip -- 3000 lines -- split by concern:
//   api.hip          context, memory, stand-alone operators (kernel matrix, gradients, GEMM, Cholesky, eigh), prediction
//   api_fit.hip      the fit handle: Lp, the n x m kernel matrix, values-in route, Gram spectrum / rank, projections
//   api_precond.hip  Gram of the row sample, whitening, Ridge / preconditioner factor, its rebuild, Ridge start
//   api_solve.hip    objective, transform, the device-resident MAP solve, predictor weights, stage times
//   api_noise.hip    FunctionEstimator: noisy landmark / full conditionals, leverage, HC3 variance weights)
// Ownership: every device or pinned block is a DevBuf (dev_buf.h) -- a member of the handle, of the context, of TriInv /
// RebuildSelection / Precond, or a local of the function that needs it.  Nothing is freed by hand; plain pointers are views.
#pragma once
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <atomic>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "linalg.h"
#include "mln_internal.h"
#include "objective.h"
#include "precond_rebuild.h"
#include "solver.h"

void fit_events_borrow(mln_ctx* ctx, std::vector<hipEvent_t>* evs);   // api_fit.hip: the context's pool of timing events
void fit_events_return(mln_ctx* ctx, std::vector<hipEvent_t>* evs);

double now_s();

// Read-only input that may live on host or device.
struct DevIn {
  mln_ctx* ctx;
  const double* dev = nullptr;
  DevBuf<double> owned;
  int init(mln_ctx* c, const double* p, size_t count) {
    ctx = c;
    if (count == 0 || !p) { dev = p; return MLN_OK; }
    if (is_device_ptr(p)) { dev = p; return MLN_OK; }
    MLN_TRY(owned.alloc(ctx, count, "device copy of an input"));
    MLN_HIP(ctx, hipMemcpyAsync(owned, p, count * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    dev = owned;
    return MLN_OK;
  }
  ~DevIn() {
    if (owned) (void)hipStreamSynchronize(ctx->stream);
  }
};

// Output that may live on host or device.
struct DevOut {
  mln_ctx* ctx;
  double* dev = nullptr;
  DevBuf<double> owned;
  double* host = nullptr;
  size_t count = 0;
  int init(mln_ctx* c, double* p, size_t n, bool copy_in = false) {
    ctx = c; count = n;
    if (n == 0) { dev = p; return MLN_OK; }
    if (is_device_ptr(p)) { dev = p; return MLN_OK; }
    host = p;
    MLN_TRY(owned.alloc(ctx, n, "device copy of an output"));
    if (copy_in) MLN_HIP(ctx, hipMemcpyAsync(owned, p, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    dev = owned;
    return MLN_OK;
  }
  int commit() {
    if (owned && count) {
      MLN_HIP(ctx, hipMemcpyAsync(host, owned, count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    MLN_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MLN_OK;
  }
  ~DevOut() {
    if (owned) (void)hipStreamSynchronize(ctx->stream);
  }
};

// ---- fit handle --------------------------------------------------------------------------------------
// The preconditioner as one value: C C^T = L^T L + I (the Ridge matrix) and C^-1, both m x ldl lower.
// Implicit ("K-space") mode factors it in w-space.  With M = s K_s^T K_s + Kj (Kj = cov(xu, xu) + jitter I = Lp Lp^T) and
// R R^T = M, the square root C = Lp^-1 R of C C^T = I + Lp^-1 (s K_s^T K_s) Lp^-T is never formed and the Gram is never
// whitened:  C holds R,  P = R^-T = Lp^-T C^-T (so that w = Lp^-T z = P u for z = C^-T u),  Cinv = C^-1 = R^-1 Lp.
// Q1 / Q2 are the stacked operators, so that one evaluation needs two row-GEMVs and no reductions:
//   Q1 = [C^-T ; P]  (2m x ldl, implicit) or C^-T (m x ldl):   [z ; w] = Q1 u
//   Q2 = [C^-1 | P^T] (m x 2 ldl, implicit) or C^-1:            g_u = Q2 [z ; K^T(a-1)]
// Stepping aside is a move, dropping is assigning a fresh Precond.
struct Precond { DevBuf<double> C, Cinv, P, Q1, Q2; };

struct mln_fit {
  mln_ctx* ctx = nullptr;
  DevCov cov;
  int d = 0;
  int64_t n = 0, m = 0, ldl = 0, ldp = 0;
  bool full = false;
  DevBuf<double> L_own;  // n x ldl
  double* L = nullptr;   // what the passes read: L_own, or Lp in the full GP (not owned)
  DevBuf<double> Lp;     // m x ldp
  TriInv tri;            // block-scaled Lp
  DevBuf<double> V, Vdr;
  double mu = 0.0;
  // objective workspace
  int n_wg = 0;
  DevBuf<double> part_grad, part_hess, part_loss;
  DevBuf<double> d_z, d_out;  // m ; 1 + 2m
  PinnedBuf<double> h_z, h_out;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  double times[MLN_N_STAGE_TIMES] = {0};
  // preconditioner (Precond above); pc_saved is the FIRST one while the solve runs on the rebuilt one: put back if that one
  // fails its trial (solver.h: revert_after), released when the solve ends
  Precond pc, pc_saved;
  DevBuf<double> d_u, d_gu, d_tmp;  // m ; m ; 1 + m
  int n_wg_cap = 0;
  // implicit ("K-space") mode: the n x m buffer holds K = cov(x, xu) itself and Lp^-T is folded
  // into the m-vectors:  L z = K (Lp^-T z),  L^T v = Lp^-1 (K^T v).  No n x m triangular solve.
  bool kspace = false;
  DevBuf<double> Kj;      // cov(xu, xu) + jitter I, full symmetric (m x ldp); implicit fits only
  // MLN_FIT_DEFER_LP: f->Lp still holds Kj; it is factored together with the preconditioner's matrix (one batched chain of
  // launches, linalg.hip dev_cholesky_lower2) or on first use (fit_ensure_lp), whichever comes first
  bool lp_pending = false, lp_failed = false, tri_pending = false;
  double jitter = 0.0;
  DevBuf<double> d_w;  // m
  // last vector pair (z, w = Lp^-T z) produced by the library itself (Ridge init / MAP solve): lets
  // mln_transform / mln_weights_cholesky on that same z skip the triangular solve
  std::vector<double> z_cached;
  DevBuf<double> d_w_cached;
  DevBuf<double> d_zw, d_zr;
  // eigenvectors of L^T L (rows, ascending eigenvalue), m x ldl: Nystroem rank reduction
  DevBuf<double> eigU;
  // fp32 copy of the streamed n x m buffer for the warm-up passes of the MAP solve (mixed precision)
  DevBuf<float> L32;
  double emu_excluded = 0.0;    // MELLON_AMD_EMULATE_RANKS: wall seconds spent on the OTHER ranks' column blocks (tools/emulate_rank.py)
  bool cov_bounded01 = false;   // every covariance value lies in [0, 1] (stationary kernels and their products)
  int l32_fixed = 0;     // format of that copy: 0 = fp32, 1 = 32-bit fixed point (covariances bounded by 1)
  int evals32 = 0;
  double times32 = 0.0;
  // evaluation buffers of the preconditioned objective: d_zr = [z (ld2) | r (ld2)] with the likelihood sum at
  // d_zr[ld2 + m] and the "rows above the solver's cap" flag at d_zr[ld2 + m + 1], so that one all-reduce of m + 2 values
  // covers [r ; lik ; over];  ld2 = pad16(m + 2)
  int64_t ld2 = 0;
  DevBuf<int> d_over;      // device word the objective kernels set when a row lay above the cap (ObjArgs::over_flag)
  int64_t row0 = 0;     // global index of this shard's first cell (subsampling is by global index)
  // device-resident L-BFGS (solver.hip)
  SolverBuffers sv{};
  DevBuf<double> sv_block;        // one allocation behind every pointer of sv
  PinnedBuf<SolverState> h_state; // pinned mirror
  int sv_maxcor = 0;
  std::vector<hipEvent_t> evs;    // three per evaluation: before the fp32 pass, between, after the fp64 pass
  // f = L z + mu of every row at the solver's accepted point, kept by the objective passes themselves
  DevBuf<double> f_keep[2];
  int f_final = -1;               // which buffer holds f at z_cached (-1: none; mln_transform then streams the buffer)
  // row subsample shared by the preconditioner's Gram and the solver's first phase: cells whose GLOBAL index is a
  // multiple of precond_stride (0: no preconditioner yet; 1: all cells)
  int64_t precond_stride = 0;
  // handle whose kernel values come from the binding (mln_fit_prepare_from_K): rows received, finished
  bool from_K = false, k_finished = false;
  int64_t k_rows_done = 0;
  int n_revert = 0, n_rebuild_skipped = 0, n_start_halvings = 0, rank_path = 0;
  double build_seconds = 0.0;     // wall time of the first preconditioner build (Gram + factorisation): the rebuild's price
  double times_sub = 0.0, times_rebuild = 0.0, sub_pass_equiv = 0.0;
  int evals_sub = 0, n_rebuild = 0;
  // importance tail of the MAP solve (solver.h): the row list drawn at the pause (alive while the solve runs), accounting
  RebuildSelection tail_sel;
  double times_tail = 0.0;
  int evals_tail = 0, n_tail_guard = 0;
  int64_t tail_rows = 0;
  // dimensionality likelihood (dimensionality.hip): ell = log(sorted k-NN distance) + log(pi) / 2 (n x dim_k), the two means,
  // the partials of one pass (n_wg x 4 ldl: both gradients, both Hessian diagonals), z and w (4 ldl), the reduced sums
  DevBuf<double> dim_ell;
  int dim_k = 0;
  double mu_dim = 0.0, mu_dens = 0.0;
  DevBuf<double> dim_part, dim_z, dim_out;
  ~mln_fit();   // api_fit.hip: drains the stream once, hands back the events; the members release themselves
};

int dev_allreduce(mln_ctx* ctx, double* dev, int64_t count);
int dev_bcast0(mln_ctx* ctx, double* dev, int64_t count);
int reject_distance_leaf(mln_ctx* ctx, const DevCov& dc);
int64_t pad16(int64_t m);
void fit_sample_rows(const mln_fit* f, int64_t s, int64_t* first, int64_t* rows);
int fit_alloc_workspace(mln_fit* f);
int fit_prepare_impl(mln_ctx* ctx, const mln_kernel_desc* cov, const double* x, int64_t n, int32_t d,
                            const double* xu, int64_t m, double jitter, const double* Lp_in, int32_t flags,
                            mln_fit* f);
ObjArgs obj_args(mln_fit* f);
void obj_account(mln_fit* f, bool f32 = false);
int fit_w_from_z(mln_fit* f, const double* z_dev, double* w_dev, const double* z_host = nullptr);
int fit_cache_pair_from_u(mln_fit* f, const double* u_dev);
int fit_enqueue_eval(mln_fit* f, const double* u_dev, double* gn_dev, bool use32, const int* gate,
                            hipEvent_t* ev, const std::vector<int64_t>* sub_strides = nullptr,
                            const RebuildSelection* tail = nullptr);
int fit_objective_u(mln_fit* f, const double* u, double* loss, double* grad_u, double* z_out,
                           bool use32 = false);
int fit_solver_alloc(mln_fit* f, int maxcor);
int gram_of(mln_ctx* ctx, const double* A, int64_t lda, int64_t rows, int64_t m, double alpha, double* G,
                   int64_t ldg, bool quantised = false);
int emulated_ranks(const mln_ctx* ctx);
int fit_ensure_kj(mln_fit* f);
int fit_ensure_lp(mln_fit* f, bool need_tri = true);   // a deferred Lp = chol(Kj) is factored now, its solve operands built (no-ops otherwise)
int fit_lp_finish(mln_fit* f, int rc_chol, double t0);   // after either route factored f->Lp: block-scaled copies, bookkeeping
// whiten = true: Lp^-1 (.) Lp^-T applied (implicit mode; a Gram whose eigenvalues are results); false: the raw K_s^T K_s
int fit_gram(mln_fit* f, double* G, int64_t ldg, int64_t row_stride, bool whiten = true);
int fit_gemvT(mln_fit* f, const double* t_dev, double* rhs_dev);
int fit_factor_precond(mln_fit* f);
int fit_build_precond(mln_fit* f, int64_t row_stride);
int fit_rebuild_precond(mln_fit* f, const double* f_dev, double rows_per_m, int* outcome, double cap = 1e300);   // outcome: 0 rebuilt, 1 weights too wild, 2 build failed (old one kept)
int fit_precond_revert(mln_fit* f);
int fit_small_gemv(mln_fit* f, const double* M, int trans, const double* w, double* y);
int launch_scale_rows_cols(mln_ctx* ctx, double* A, int64_t ld, int64_t rows, int64_t cols, const double* row,
                                  const double* col);
// sparse_targets.hip: 2-D targets kept in CSR (host arrays the entry has validated; nnz = indptr[n]).
struct CsrTargets { const int64_t* indptr; const int32_t* indices; const double* data; int64_t nnz; };
// C (m x p, ldc = p) = alpha * L^T (y - mu), L = n x m with pitch ldl, from row panels of y - mu built in HBM
int csr_targets_product(mln_ctx* ctx, const double* L, int64_t ldl, int64_t m, int64_t n, int64_t p,
                        const CsrTargets& y, double mu, double alpha, double* C);
// y: dense n_local x p, or NULL with `csr` set
int sparse_solve_impl(mln_ctx* ctx, const mln_kernel_desc* cov, const double* x, int64_t n_local,
                             int32_t d, const double* xu, int64_t m, const double* y, int64_t p, double mu,
                             const double* sigmas, int32_t kind, double jitter, double* W, double* Lp_out,
                             double* Cs_out, const CsrTargets* csr = nullptr);
unsigned grid_1d(int64_t count);
