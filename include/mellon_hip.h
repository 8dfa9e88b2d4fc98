/*
 * mellon_hip.h -- C ABI of libmellon_hip.so, the MI355X (gfx950) sparse-GP density core.
 *
 * The reference (settylab/Mellon v1.7.1) has NO native code: its hot path is Python on
 * JAX/XLA:CPU.  Each entry point below replaces the arithmetic of the reference function(s)
 * cited next to it (paths relative to the reference checkout), so that the reference's
 * estimator classes -- or this repo's mirror of them, mellon_amd/ -- can bind it with ctypes.
 * INTEGRATION.md shows the reference-side stubs.
 *
 * Conventions
 *   - all matrices are row-major float64; sizes are int64_t, feature counts int32_t;
 *   - every data pointer may be a HOST pointer or a DEVICE pointer obtained from mln_malloc():
 *     the library detects which (hipPointerGetAttributes) and stages host buffers itself;
 *   - the caller owns every buffer it passes; the library owns what sits behind mln_ctx /
 *     mln_fit handles; no pointer is retained after a call returns except inside a handle;
 *   - every function returns an mln_status (0 = ok); no C++ exception crosses the ABI;
 *     mln_last_error() gives the text.  MLN_ERR_NOT_PD maps to the reference's
 *     ValueError("Covariance not positively definite with jitter=...") (decomposition.py:116-122);
 *   - a mln_ctx is bound to one GPU and is not thread-safe; calls are synchronous on return;
 *   - there is no CPU fallback: without a usable gfx950 device mln_ctx_create fails.
 */
#ifndef MELLON_HIP_H
#define MELLON_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mln_ctx mln_ctx;
typedef struct mln_fit mln_fit;

typedef enum {
  MLN_OK = 0,
  MLN_ERR_NOT_PD = 1,      /* non-positive / NaN pivot in a Cholesky factorisation          */
  MLN_ERR_SHAPE = 2,       /* inconsistent sizes                                            */
  MLN_ERR_HIP = 3,         /* HIP runtime failure (text in mln_last_error)                  */
  MLN_ERR_RCCL = 4,        /* RCCL failure                                                  */
  MLN_ERR_ARG = 5,         /* null pointer / bad enum / unsupported descriptor              */
  MLN_ERR_UNSUPPORTED = 6, /* valid request this build cannot serve (e.g. m too large)      */
  MLN_ERR_NOCONV = 7       /* an iterative kernel (Jacobi eigensolver) did not converge     */
} mln_status;

/* ---- kernel-plugin surface: mellon/base_cov.py:17-497 + mellon/cov.py ------------------- */
typedef enum {
  MLN_K_MATERN32 = 1,    /* cov.py:62-66   */
  MLN_K_MATERN52 = 2,    /* cov.py:157-161 */
  MLN_K_EXPQUAD = 3,     /* cov.py:255-259 */
  MLN_K_EXPONENTIAL = 4, /* cov.py:352-356 */
  MLN_K_RATQUAD = 5,     /* cov.py:453-457 */
  MLN_K_LINEAR = 6,      /* cov.py:551-556 */
  MLN_K_DISTANCE = 7     /* util.py:351-366: the pairwise distance itself, dist / ls (values only, no gradients) */
} mln_kind;

/* A covariance tree (Covariance / Add / Mul / Pow, base_cov.py:301-453) is lowered to a postfix
 * program over leaves.  Each leaf carries the FINAL column indices it sees after every enclosing
 * `active_dims` selection has been composed (util.py:150-171).                                 */
typedef struct {
  int32_t kind;        /* mln_kind                                        */
  int32_t ndims;       /* number of active columns                        */
  double ls;           /* length scale                                    */
  double alpha;        /* RatQuad only                                    */
  const int32_t* dims; /* ndims column indices into the d input columns   */
} mln_leaf;

typedef enum { MLN_OP_LEAF = 0, MLN_OP_CONST = 1, MLN_OP_ADD = 2, MLN_OP_MUL = 3, MLN_OP_POW = 4 } mln_op;

typedef struct {
  int32_t op;   /* mln_op                                   */
  int32_t leaf; /* MLN_OP_LEAF: index into leaves           */
  double value; /* MLN_OP_CONST: the scalar                 */
} mln_tok;

#define MLN_MAX_LEAVES 4
#define MLN_MAX_TOKS 16
#define MLN_MAX_DIMS 256 /* total over all leaves */

typedef struct {
  int32_t n_leaves;
  int32_t n_toks;
  const mln_leaf* leaves;
  const mln_tok* toks;
} mln_kernel_desc;

/* ---- context / memory ------------------------------------------------------------------- */
int mln_ctx_create(int device, mln_ctx** out);
void mln_ctx_destroy(mln_ctx* ctx);
const char* mln_last_error(mln_ctx* ctx); /* ctx may be NULL: last error of the calling thread */
int mln_device_info(mln_ctx* ctx, char* name, int name_cap, int* n_cu, int64_t* mem_bytes);
int mln_device_count(int* count_out); /* GPUs visible to this process (0 and MLN_OK when there are none) */
int mln_synchronize(mln_ctx* ctx);

int mln_malloc(mln_ctx* ctx, int64_t bytes, void** dev_ptr);
int mln_free(mln_ctx* ctx, void* dev_ptr);
int mln_memcpy(mln_ctx* ctx, void* dst, const void* src, int64_t bytes); /* any host/device mix */
/* Page-lock a HOST array of the caller (hipHostRegister) so that the library's uploads from it are DMA transfers that run
 * under its kernels: the reference's timed region starts from X in host memory (density_estimator.py:542-581), and from
 * pageable memory ~11 ms of C3's 0.4 GB upload stay exposed.  Registration itself costs ~0.1 ms per MB: once per array,
 * not per fit.  The caller unregisters before freeing the array.  Both return MLN_ERR_HIP when the runtime refuses.   */
int mln_host_register(mln_ctx* ctx, const void* host_ptr, int64_t bytes);
int mln_host_unregister(mln_ctx* ctx, const void* host_ptr);
/* Internal buffers (the 8*n*m-byte factor, Gram partials, ...) are recycled by a caching
 * allocator so that repeated fits do not pay hipMalloc / page-mapping again; this returns all
 * cached blocks to the driver.                                                                */
int mln_release_cached_memory(void);
/* Read-only view of that allocator (process-wide, no context): out[0] device blocks handed out and not yet released,
 * out[1] their bytes as recorded, out[2] pinned host blocks handed out, out[3] bytes sitting in the device cache,
 * out[4] successful hipMalloc calls since load.  Memory from mln_malloc is not counted.       */
int mln_diag_alloc_stats(int64_t* out);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI ------------------------------------------
 * Cells (rows of x) are sharded; landmarks, Lp and z are replicated.  Collectives: all-reduce
 * of (loss, grad) per objective evaluation and of the m x m Ridge Gram once per fit.          */
#define MLN_UNIQUE_ID_BYTES 128
int mln_comm_unique_id(void* id_out /* MLN_UNIQUE_ID_BYTES */);
int mln_comm_init(mln_ctx* ctx, const void* id, int n_ranks, int rank);
int mln_comm_allreduce_sum(mln_ctx* ctx, double* buf, int64_t count); /* host or device buffer */
/* Loopback communicator: n_ranks contexts of ONE process (one host thread per rank; the contexts may all sit
 * on the same GPU) exchange through device memory and a host barrier, every rank summing the contributions in
 * rank order.  Same call sites, same results as RCCL -- it runs the N-rank sharded path on a single GPU.
 * Every rank must enter each collective; the group outlives the contexts attached to it.                       */
typedef struct mln_loopback mln_loopback;
int mln_loopback_create(int n_ranks /* <= 16 */, mln_loopback** out);
void mln_loopback_destroy(mln_loopback* group);
int mln_comm_init_loopback(mln_ctx* ctx, mln_loopback* group, int rank);
/* Host-staged collectives: the fall-back for a box where RCCL cannot be initialised, and the way to run the real
 * multi-PROCESS path on fewer GPUs than ranks (RCCL refuses two ranks on one device).  The library copies the buffer to
 * pinned host memory, calls `fn`, copies the result back, all in stream order.  op 0: all-reduce (sum over ranks, in rank
 * order) of buf[count] in place; op 1: buf[count] <- rank 0's; op 2: all-gather, buf[count] of every rank in rank order
 * into buf2[n_ranks * count].  fn returns 0 on success. */
typedef int (*mln_host_collective_fn)(void* user, int op, double* buf, double* buf2, int64_t count);
int mln_comm_init_host(mln_ctx* ctx, int n_ranks, int rank, mln_host_collective_fn fn, void* user);
void mln_loopback_abort(mln_loopback* group); /* a rank failed outside a collective: wake the others with MLN_ERR_RCCL */
/* What the communicator of `ctx` is and what it has carried (no counterpart in the reference, which has no distributed
 * code: this is how a multi-GPU bench line proves which transport ran -- SURVEY.md S8(e)).
 *   info[4]  (nullable): transport 0 none / 1 RCCL / 2 in-process loopback / 3 host-staged; the rank count and the rank
 *            AS THE TRANSPORT REPORTS THEM (ncclCommCount / ncclCommUserRank for RCCL; -1 if it cannot say); RCCL's
 *            version code (0: not loaded).
 *   stats[10] (nullable): calls, bytes of all-reduce | broadcast | all-gather since the last reset; the all-reduces of
 *            <= 64 KB among them (the per-evaluation [grad ; loss]); event-timed milliseconds of the LARGE all-reduces,
 *            of broadcasts + all-gathers, of the small all-reduces (0 unless timing is on; reading them synchronises).
 *   flags:   1 = timing on (a pair of stream events around every collective), 2 = off, 4 = reset counters afterwards. */
int mln_comm_info(mln_ctx* ctx, int32_t* info, double* stats, int32_t flags);

/* ---- a-1..a-3: K = cov(x, y)   (util.py:351-366 distance, cov.py k(), base_cov.py Add/Mul/Pow)
 * x: n x d, y: m x d, out: n x m.                                                              */
int mln_kernel_matrix(mln_ctx* ctx, const mln_kernel_desc* cov, const double* x, int64_t n,
                      const double* y, int64_t m, int32_t d, double* out);

/* ---- feeding the path (S8f rank 1): exact Euclidean nearest-neighbour distance of each row of x
 * (n x d) among the rows of y (m x d), excluding the pair (i, i + self_offset) -- pass y = x and
 * self_offset = 0 for the estimator's nn_distances (parameters.py:408-433; the reference's
 * pynndescent search is approximate), or y = all cells and self_offset = shard start when sharded. */
/* cov(x, xu)^T cov(x, xu) (m x m), summed over the ranks' shards: the B^T B of the landmark leverage
 * diag(B M^-1 B^T), M = sigma^2 K_uu + B^T B + jitter I (conditional.py:593-601,660-685). */
int mln_kernel_gram(mln_ctx* ctx, const mln_kernel_desc* cov, const double* x, int64_t n_local, int32_t d,
                    const double* xu, int64_t m, double* out /* m x m */);
int mln_nn_distances(mln_ctx* ctx, const double* x, int64_t n, const double* y, int64_t m, int32_t d,
                     int64_t self_offset, double* out /* n */);
/* Exact k nearest neighbours (dimensionality_estimator.py:377-394 via parameters.py:352-405, util.py:486-536): for each
 * row of x (n x d) the k rows of y (m x d) nearest in Euclidean distance, ascending, ties broken by the smaller index;
 * with exclude != 0 the pair (i, i + self_offset) is skipped (as in mln_nn_distances).  1 <= k <= 64, k <= m (k <= m - 1
 * with exclude), any d.  dist: n x k, sqrt(sum (x - y)^2) in fp64 (difference form: close neighbours keep their digits);
 * idx: n x k (may be NULL).  O(n k) working memory (csrc/dimensionality.hip). */
int mln_knn(mln_ctx* ctx, const double* x, int64_t n, const double* y, int64_t m, int32_t d, int32_t k,
            int32_t exclude, int64_t self_offset, double* dist /* n x k */, int64_t* idx /* n x k or NULL */);
/* Local fractal dimension (util.py:486-536): for query i, the k rows x[nbr[i, :]] (2 <= k <= 64), their k(k-1)/2 pair
 * distances sorted ascending, and the least-squares slope of log(1 .. k(k-1)/2) on [log(distance), 1] in closed form.
 * A zero pair distance gives NaN for that query (as lstsq on log 0). x: n x d, nbr: q x k (host or device). */
int mln_local_dimensionality(mln_ctx* ctx, const double* x, int64_t n, int32_t d, const int64_t* nbr, int64_t q,
                             int32_t k, double* out /* q */);

/* k-means landmarks (S8f rank 1): k-means++ seeding + Lloyd sweeps on the device, the algorithm
 * family of sklearn.cluster.k_means(x, m, n_init=1, random_state) that parameters.compute_landmarks
 * calls (parameters.py:275-291).  Own RNG stream / summation order: centroids are equivalent in
 * quality, not bit-compatible with sklearn.  d <= 64.  centers: m x d.  The sweeps carry Hamerly's
 * distance bounds (same assignments, searched only where the bounds do not decide).  n_iter_out and
 * inertia_out may be NULL; the inertia is a full fp64 assignment of all cells to the final centres. */
int mln_kmeans(mln_ctx* ctx, const double* x, int64_t n, int32_t d, int64_t m, int64_t seed,
               int32_t max_iter, double tol, double* centers, int32_t* n_iter_out, double* inertia_out);
/* The same with sklearn's OWN seeding (sklearn.cluster._kmeans._kmeans_plusplus behind k_means(x, m, n_init=1,
 * random_state), parameters.py:275-291): the first centre is cell `first_id`, centre c is the best of n_local_trials
 * (= 2 + int(log m)) candidates drawn at uniforms[(c - 1) * n_local_trials + l] * current_pot on the cumulative sums of the
 * squared distances.  The caller draws first_id and the (m - 1) * n_local_trials uniforms with numpy's
 * RandomState(random_state) -- exactly the numbers sklearn consumes -- so the seeds are the cells sklearn picks (up to
 * summation order: see csrc/kmeans.hip) and the landmarks comparable with the reference's at any size.  Lloyd's sweeps
 * then run over all cells to sklearn's stopping rule; max_iter = 0 returns the seeds.  indices_out (m, may be NULL): the
 * seeded cells. */
int mln_kmeans_sklearn(mln_ctx* ctx, const double* x, int64_t n, int32_t d, int64_t m, int64_t first_id,
                       const double* uniforms, int32_t n_local_trials, int32_t max_iter, double tol, double* centers,
                       int64_t* indices_out, int32_t* n_iter_out, double* inertia_out);

/* ---- a-4/a-5: in-place lower Cholesky of (A + add_diag * I), A m x m symmetric (lower read).
 * decomposition.py:111-123 (`stabilize` util.py:269-293 + jnp.linalg.cholesky).  Strict upper
 * triangle of the result is zero.  MLN_ERR_NOT_PD on a non-positive or NaN pivot.              */
int mln_chol_lower(mln_ctx* ctx, double* A, int64_t m, double add_diag);

/* triangular solves with a lower factor Lf (m x m):  B (m x p) <- op(Lf)^-1 B.
 * trans = 0: Lf^-1 B (solve_triangular(L, B, lower=True)); trans = 1: Lf^-T B
 * (solve_triangular(L.T, B)), conditional.py:63-65,264,818.                                    */
int mln_trsm_lower(mln_ctx* ctx, const double* Lf, int64_t m, int32_t trans, double* B, int64_t p);

/* ---- fit handle: device-resident shard state --------------------------------------------------
 * mln_fit_prepare follows parameters.compute_Lp (parameters.py:648-714) and compute_L
 * (parameters.py:783-874):
 *   xu != NULL (sparse_cholesky): Lp = chol(cov(xu,xu) + max(sigma^2,jitter) I)  decomposition.py:111-123
 *                                 L  = cov(x,xu) Lp^-T                           decomposition.py:205-210
 *   xu == NULL (full):            Lp = chol(cov(x,x) + jitter I);  L = Lp        parameters.py:847-850
 * Lp_in (optional, m x m) skips the factorisation (the estimator's `Lp=` ctor argument).
 * x is THIS RANK's shard (n_local x d); with a communicator the full-GP branch is refused.    */
#define MLN_FIT_IMPLICIT 1 /* flags: keep K = cov(x,xu) in the n x m buffer and fold Lp^-T into the
                             m-vectors (L z = K (Lp^-T z), L^T v = Lp^-1 (K^T v)): no n x m triangular
                             solve; mln_fit_get_L materialises rows on demand; no Hessian diagonal.
                             For n_local * m >= 2^27 the kernel-matrix pass also keeps a 32-bit copy of K
                             (n_local x ld x 4 bytes: fixed point round(v 2^32) when the covariance is a stationary
                             kernel or a product of such, i.e. bounded by 1; fp32 otherwise) for the warm-up passes of
                             mln_map_solve, which finishes on the fp64 buffer at the same tolerances; environment
                             MELLON_AMD_MIXED=0 disables, MELLON_AMD_MIXED_MIN_ELEMS moves the threshold. */
int mln_fit_prepare(mln_ctx* ctx, const mln_kernel_desc* cov, const double* x, int64_t n_local,
                    int32_t d, const double* xu, int64_t m, double jitter, const double* Lp_in,
                    int32_t flags, mln_fit** out);
/* Adopt factors computed elsewhere (the estimator's `L=` / `Lp=` ctor arguments,
 * density_estimator.py:180-205): L is n_local x m; Lp (m x m) may be NULL, in which case the
 * predictor-weight entries are unavailable on this handle.                                      */
int mln_fit_from_L(mln_ctx* ctx, const double* L, int64_t n_local, int64_t m, const double* Lp,
                   mln_fit** out);
/* ---- kernel-plugin surface, user-defined kernels: a Covariance subclass whose k(x, y) is Python code
 * (base_cov.py:17-69: the ABC's only contract is `k`) cannot be lowered to an mln_kernel_desc.  The binding then
 * evaluates the USER'S function itself -- cov(xu, xu) once, cov(x_block, xu) in row blocks -- and hands the values
 * over; everything after the kernel matrix (Cholesky, triangular solves, Ridge, MAP solve, weights) is the same
 * device path as for the built-in kernels.  The same entries serve covariance trees too large for one device
 * program (MLN_MAX_LEAVES / MLN_MAX_TOKS), whose blocks the binding assembles on the device with mln_ewise.
 *   mln_fit_prepare_from_K  Kuu = cov(xu, xu) (m x m; jitter is added here; ignored when Lp_in is given);
 *                           flags: MLN_FIT_IMPLICIT as above; MLN_FIT_FULL: the full GP (n_local == m, L = Lp,
 *                           no n x m buffer, nothing to upload)
 *   mln_fit_set_K_rows      rows [row0, row0 + n_rows) of cov(x, xu), n_rows x m, host or device
 *   mln_fit_finish_K        after the last block: L = K Lp^-T unless implicit; the handle is then a normal fit     */
#define MLN_FIT_FULL 2
/* MLN_FIT_DEFER_LP (with MLN_FIT_IMPLICIT, no Lp given): Lp = chol(cov(xu, xu) + jitter I) is not factored inside
 * mln_fit_prepare but together with the preconditioner's matrix in mln_precond_build / mln_ridge_init (two
 * factorisations in one chain of launches), or by the first call that needs it; MLN_ERR_NOT_PD then comes from
 * that call, its message starting with "cov(xu, xu)". */
#define MLN_FIT_DEFER_LP 4
int mln_fit_prepare_from_K(mln_ctx* ctx, const double* Kuu, int64_t n_local, int64_t m, double jitter,
                           const double* Lp_in, int32_t flags, mln_fit** out);
int mln_fit_set_K_rows(mln_fit* fit, int64_t row0, int64_t n_rows, const double* K_rows);
int mln_fit_finish_K(mln_fit* fit);
/* C (M x N) = alpha op(A) op(B) + beta C on the fp64 matrix cores; row-major, host or device pointers.
 * ta = 0: A is M x K (lda >= K); ta = 1: A is stored K x M.  tb likewise.  The mean of a predictor with a
 * user-defined kernel is mu + cov(Xnew, centers) W with the kernel block evaluated by the user's k
 * (conditional.py:366-373,651-658,899-906).                                                                       */
int mln_gemm(mln_ctx* ctx, int32_t ta, int32_t tb, int64_t M, int64_t N, int64_t K, double alpha, const double* A,
             int64_t lda, const double* B, int64_t ldb, double beta, double* C, int64_t ldc);
/* out[i] = a[i] op (b ? b[i] : scalar), op in {MLN_OP_ADD, MLN_OP_MUL, MLN_OP_POW} (base_cov.py:309-315,375-381,
 * 449-453 on whole blocks); out may alias a.  Device or host pointers.                                            */
int mln_ewise(mln_ctx* ctx, int32_t op, const double* a, const double* b, double scalar, double* out, int64_t count);

void mln_fit_destroy(mln_fit* fit);
int mln_fit_get_Lp(mln_fit* fit, double* out /* m x m */);
int mln_fit_get_L(mln_fit* fit, int64_t row0, int64_t n_rows, double* out /* n_rows x m */);
int mln_fit_rank(mln_fit* fit, int64_t* m_out); /* number of columns of L */

/* ---- analytic gradients ---------------------------------------------------------------------------
 * mln_kernel_grad: Covariance.k_grad (cov.py:68-100,163-202,261-299,358-396,459-499,558-596 and the
 * Add/Mul/Pow rules of base_cov.py:317-497): out[i][j][:] = d cov(x_i, y_j) / d y_j, zero on inactive
 * dims, with util.distance_grad's denominator (dist + 1e-12) (util.py:416-423).
 * mln_predict_gradient: Predictor.gradient (base_predictor.py:490-505 -> derivatives.gradient, the
 * jax.jacrev of `_mean`): out[i][:] = sum_j W[j] d cov(x_i, c_j) / d x_i, the exact derivative of the
 * mean mln_predict_mean evaluates (denominator dist); the n x m x d tensor is never formed.          */
int mln_kernel_grad(mln_ctx* ctx, const mln_kernel_desc* cov, const double* x, int64_t n, const double* y,
                    int64_t m, int32_t d, double* out /* n x m x d */);
int mln_predict_gradient(mln_ctx* ctx, const mln_kernel_desc* cov, const double* xnew, int64_t n_new,
                         int32_t d, const double* centers, int64_t m, const double* W /* m */,
                         double* out /* n_new x d */);
/* The same for a predictor with p outputs (FunctionEstimator on p columns; the time grid of PredictorTime with the time
 * factor folded into the weights): out[i][q][:] = sum_j W[j][q] d cov(x_i, c_j) / d x_i.  p == 1 is mln_predict_gradient
 * bit for bit.  Stationary leaves and n_new m >= 2^16: the coefficient matrices (dP/dk_l) g_l are written once per row
 * chunk WITHOUT weights, and blocks of outputs are contracted by one GEMM per leaf against [W_q C|dims_l, W_q] -- the
 * covariance epilogue runs once per (row, centre) pair, whatever p is.  Otherwise (a Linear leaf, fewer pairs) column by
 * column through the single-output routes, with their bits.                                                          */
int mln_predict_gradient_multi(mln_ctx* ctx, const mln_kernel_desc* cov, const double* xnew, int64_t n_new, int32_t d,
                               const double* centers, int64_t m, const double* W /* m x p, row-major */, int64_t p,
                               double* out /* n_new x p x d */);
/* Hessian of the mean at every row of xnew, out: n_new x d x d (base_predictor.py:507-521: jacfwd(jacrev(_mean));
 * here the closed-form second derivatives of the kernels, contracted with the weights on the matrix cores).      */
int mln_predict_hessian(mln_ctx* ctx, const mln_kernel_desc* cov, const double* xnew, int64_t n_new, int32_t d,
                        const double* centers, int64_t m, const double* W /* m */, double* out);
/* The same for p outputs: out[i][q] = the Hessian of output q at row i.  p == 1 is mln_predict_hessian bit for bit, and so
 * is, column by column, a call with n_new m < 2^16.  Otherwise, for any program (Linear factors included), the coefficient
 * matrices are written once per row chunk WITHOUT weights and blocks of outputs are contracted by one GEMM per leaf pair
 * against W_q [vec(c c'^T) | c | c' | 1], the diagonal term by one GEMM against the weights themselves.  A zero column of W and
 * inactive dims give exact zeros.                                                                                        */
int mln_predict_hessian_multi(mln_ctx* ctx, const mln_kernel_desc* cov, const double* xnew, int64_t n_new, int32_t d,
                              const double* centers, int64_t m, const double* W /* m x p, row-major */, int64_t p,
                              double* out /* n_new x p x d x d */);
/* numpy.linalg.slogdet of the leading lead x lead block (1 <= lead <= k) of `count` row-major k x k matrices lda >= k k doubles
 * apart: LU with partial pivoting (ties to the lowest row), sign in {-1, 0, +1}, a singular block gives (0, -inf).  Host or
 * device pointers.  lead > 64 is MLN_ERR_UNSUPPORTED.  Non-finite entries are outside the contract.                      */
int mln_slogdet_batched(mln_ctx* ctx, const double* A, int64_t count, int32_t k, int64_t lda, int32_t lead,
                        double* sign /* count */, double* logabsdet /* count */);
/* mln_predict_hessian_multi followed by mln_slogdet_batched without the Hessians leaving the device (they are built and
 * factored per row chunk and block of outputs in scratch): Predictor.hessian_log_determinant (base_predictor.py:523-539;
 * lead = d) and PredictorTime's (1162-1194; lead = d - 1, the state columns).  The Hessians factored are, bit for bit,
 * those mln_predict_hessian_multi returns.                                                                             */
int mln_predict_hessian_logdet(mln_ctx* ctx, const mln_kernel_desc* cov, const double* xnew, int64_t n_new, int32_t d,
                               const double* centers, int64_t m, const double* W /* m x p, row-major */, int64_t p,
                               int32_t lead, double* sign /* n_new x p */, double* logabsdet /* n_new x p */);

/* ---- derivatives of block-evaluated covariance trees (more than MLN_MAX_LEAVES leaves, a deeper stack, user-defined
 * leaves; base_cov.py:317-497, base_predictor.py:490-539).  The binding walks the tree per row block and carries every
 * node's value and its first / second derivatives with respect to the leaves as (n x ld) device blocks (mln_ewise);
 * these entries supply the leaf factors and contract the finished coefficient blocks.  For a stationary leaf
 * grad_x k = g (x - c)|dims and hess_x k = g I|dims + h (x - c)(x - c)^T|dims; for Linear grad_x k = c|dims / ls.
 *   mln_leaf_factors           K, g and (h != NULL) h of ONE built-in leaf (a one-leaf descriptor), n x ld each, columns
 *                              m .. ld - 1 zero; the same device arithmetic as mln_kernel_matrix / mln_predict_gradient /
 *                              mln_predict_hessian.  exact_denominator = 1: g = phi'(dist) / dist, 0 where the distance clamp
 *                              is active (derivatives of the mean); 0: util.distance_grad's dist + 1e-12 (k_grad).  For a
 *                              Linear leaf g = 1 / ls and h = 0.
 *   mln_block_grad_accumulate  out[i][:] = sum_l sum_j Q_l[i][j] w_j (x_i - c_j)|dims_l  (Linear: ... w_j c_j|dims_l),
 *                              Q_l = (dP/dk_l) g_l: one GEMM per leaf against [w C|dims_l, w].  out: n x d.
 *   mln_block_hess_accumulate  out[i] = sum_l diag_l(sum_j w_j Qd_l[i][j]) + sum_{l <= l'} sum_j w_j Qp_ll'[i][j] S(dl dl'^T),
 *                              dl = (sig_l x_i - c_j)|dims_l (sig = 0 for Linear), S = the product plus its transpose when
 *                              l != l'.  Qd_l = a_l g_l (stationary leaves; NULL: none), Qp in the order (0,0) (0,1) ..
 *                              (0,L-1) (1,1) ..: a_l h_l + a_ll gam_l^2 on the diagonal, a_ll' gam_l gam_l' off it (gam = g,
 *                              or -1 / ls for Linear); NULL entries are identically zero.  out: n x d x d.
 *   mln_block_kernel_grad      out[i][j][:] = sum_l A_l[i][j] (y_j - x_i)|dims_l  (Linear: A_l[i][j] x_i|dims_l): the k_grad
 *                              of the tree with A_l = (dP/dk_l) g_l.  out: n x m x d.
 * Coefficient blocks are DEVICE pointers with row pitch ld >= m; x, y / centers, w, out may be host or device.     */
int mln_leaf_factors(mln_ctx* ctx, const mln_kernel_desc* leaf, const double* x, int64_t n, const double* y, int64_t m,
                     int32_t d, int32_t exact_denominator, int64_t ld, double* K, double* g, double* h /* or NULL */);
int mln_block_grad_accumulate(mln_ctx* ctx, const mln_leaf* leaves, int32_t n_leaves, const double* const* Q, int64_t ld,
                              const double* x, int64_t n, int32_t d, const double* centers, int64_t m,
                              const double* w /* m */, double* out /* n x d */);
int mln_block_hess_accumulate(mln_ctx* ctx, const mln_leaf* leaves, int32_t n_leaves, const double* const* Qd,
                              const double* const* Qp, int64_t ld, const double* x, int64_t n, int32_t d,
                              const double* centers, int64_t m, const double* w /* m */, double* out /* n x d x d */);
int mln_block_kernel_grad(mln_ctx* ctx, const mln_leaf* leaves, int32_t n_leaves, const double* const* A, int64_t ld,
                          const double* x, int64_t n, const double* y, int64_t m, int32_t d, double* out /* n x m x d */);


/* ---- Nystroem rank reduction (decomposition.py:23-76,126-171,213-266) ---------------------------
 * mln_eigh replaces jax.numpy.linalg.eigh at decomposition.py:50 (_eigendecomposition): A (m x m,
 * symmetrised as (A + A^T)/2 like jax's symmetrize_input default) -> w (m, ascending) and V (m x m
 * row-major, COLUMN j = eigenvector j; sign of each column is arbitrary as in LAPACK).  Block
 * one-sided Jacobi on the device; MLN_ERR_NOCONV if 40 sweeps do not orthogonalise.
 *
 * _modified_low_rank (:213-266: QR of C = cov(x,xu), eigh of W = cov(xu,xu)+sigma2 I, eigh of
 * R W^-1 R^T, L = Q V sqrt(S)) is computed through the identity  L L^T = B U_p U_p^T B^T  with
 * B = C Lp^-T (the factor of an explicit mln_fit_prepare handle, Lp Lp^T = W) and (S, U) the
 * eigenpairs of the m x m Gram B^T B = Lp^-1 C^T C Lp^-T  (same non-zero spectrum as R W^-1 R^T):
 *   mln_fit_gram_eigh : S (m, ascending) to the host, U kept in the handle   [all-reduce of the Gram]
 *   mln_fit_project   : new handle with L = B U[:, m-p:]  (n_local x p; columns ordered like the
 *                       reference's s[-p:], v[:, -p:]; column signs arbitrary)
 * The rank rule of _eigendecomposition (:51-76) is host logic on S (mellon_amd/decomposition.py).   */
int mln_eigh(mln_ctx* ctx, const double* A, int64_t m, double* w, double* V, int32_t* n_sweeps);
int mln_fit_gram_eigh(mln_fit* fit, double* w /* m */, int32_t* n_sweeps);
/* util.test_rank (util.py:429-483) = numpy.linalg.matrix_rank(L, rtol=tol): the number of singular values of L above
 * tol * the largest, i.e. of eigenvalues of L^T L (all cells, all ranks) above tol^2 * lambda_max -- counted by Sturm
 * sequences on the Householder-tridiagonalised Gram, no eigendecomposition.  sigma_max_out may be NULL. */
int mln_fit_gram_rank(mln_fit* fit, double tol, int64_t* rank_out, double* sigma_max_out);
int mln_fit_project(mln_fit* fit, int64_t p, mln_fit** out);

/* a-9: Ridge initial value  z0 = (L^T L + I)^-1 L^T target   (parameters.py:877-896;
 * sklearn Ridge(alpha=1, fit_intercept=False)).  target: n_local.  All-reduced over ranks.     */
int mln_ridge_init(mln_fit* fit, const double* target, double* z0 /* m */);

/* Preconditioned MAP variable (no counterpart in the reference, which runs L-BFGS-B on z directly):
 * with C C^T = L^T L + I -- the Ridge matrix above, which equals the MAP Hessian wherever
 * exp(f + V) = 1 -- the substitution z = C^-T u makes the strictly convex objective well conditioned,
 * so the same optimiser reaches the same unique optimum in ~10x fewer passes over L.
 *   mln_precond_build      factor C and C^-1 (done implicitly, from all cells, by mln_ridge_init).  Any SPD
 *                          matrix preconditions a strictly convex problem: estimating the Gram from every
 *                          row_stride-th cell (~8 m rows suffice) costs 1/row_stride of the n m^2 flops
 *   mln_precond_apply      mode 0: u = C^T z;  mode 1: z = C^-T u;  mode 2: g_u = C^-1 g_z   (host m-vectors)
 *   mln_objective_precond  loss(C^-T u) and its gradient in u; optionally also z = C^-T u      */
int mln_precond_build(mln_fit* fit, int64_t row_stride /* Gram from every row_stride-th cell; 1 = all */);
/* Cell-sharded fits: the global index of this shard's first cell (default 0).  The row subsample above takes the cells
 * whose GLOBAL index is a multiple of row_stride, so the preconditioner does not depend on the sharding.             */
int mln_fit_set_row_offset(mln_fit* fit, int64_t global_row0);
int mln_precond_apply(mln_fit* fit, int32_t mode, const double* in, double* out);
int mln_objective_precond(mln_fit* fit, const double* u, double* loss, double* grad_u /* m */,
                          double* z_out /* m or NULL */);

/* a-7: nearest-neighbour likelihood constants of this shard (inference.py:83-85), computed by
 * the caller from nn_distances and d:  V = d log r + c,  Vdr = log d + (d-1) log r + c.        */
int mln_fit_set_likelihood(mln_fit* fit, const double* V, const double* Vdr, double mu);

/* a-7 (+ a-14): loss(z) = 1/2 |z|^2 + (m/2) log 2pi - sum_i [f_i + Vdr_i - exp(f_i + V_i)],
 * f = L z + mu (inference.py:35-92,167-192), its gradient z + L^T (exp(f+V) - 1), and optionally
 * the diagonal of the Hessian 1 + sum_i L_ij^2 exp(f_i+V_i) (inference.py:291-338 in closed form).
 * One pass over L.  Sums are all-reduced over ranks; prior terms are added once.               */
int mln_objective(mln_fit* fit, const double* z, double* loss, double* grad /* m */,
                  double* hess_diag /* m or NULL */);

/* mln_objective at S points in one call (the Monte-Carlo step of optimizer="advi", inference.py:768-876):
 * loss[s], grad[s][:] = mln_objective(fit, Z[s][:]).  Z, grad: S x m row-major (row s = sample s); loss: S.  Any S >= 1
 * (chunks of 64 samples inside).  Same likelihood (mln_fit_set_likelihood), same all-reduce over ranks (one per chunk:
 * the losses and the gradient block together), prior terms added once per sample.  No likelihood cap; a non-finite loss
 * is returned as it comes.  Two passes over the n x m buffer per chunk instead of one per sample: F = B W and
 * G = B^T (exp(F + mu + V) - 1) on the fp64 matrix cores (csrc/objective_batch.hip).  Every handle layout is batched:
 * explicit and implicit factors, Nystroem projections, mln_fit_from_L, the full GP, any number of landmarks.
 * Bit-reproducible from call to call. */
int mln_objective_batch(mln_fit* fit, const double* Z, int32_t S, double* loss /* S */, double* grad /* S x m */);

/* a-8: the MAP solve.  inference.minimize_lbfgsb (inference.py:272-288) is SciPy's L-BFGS-B without
 * bounds behind jaxopt.ScipyMinimize; this is the same limited-memory BFGS with the same stopping
 * tests (relative loss decrease <= ftol, max|grad| <= gtol, maxiter), run inside the library on the
 * preconditioned variable so that one evaluation = one device pass with no host framework in between.
 * status: 0 converged, 1 maxiter, 2 line search failed; + 4 when a solve that did NOT converge stopped with cells above the
 * likelihood cap (its loss / gradient are then the capped objective's, a minorant of inference.py:35-92's).   */
typedef struct {
  int32_t maxiter; /* 5000  */
  int32_t maxcor;  /* 10    L-BFGS memory (<= 64)    */
  int32_t maxls;   /* 30    line-search evaluations  */
  double ftol;     /* 1e-13 (SciPy default 2.2e-9 leaves the log-density ~5e-5 off the optimum) */
  double gtol;     /* 1e-7  on the preconditioned gradient */
} mln_solver_opts;
int mln_map_solve(mln_fit* fit, const double* z0, const mln_solver_opts* opts /* NULL = defaults */,
                  double* z_out /* m */, double* loss_out, int32_t* n_eval_out, int32_t* n_iter_out,
                  int32_t* status_out);

/* DimensionalityEstimator likelihood (inference.py:95-122,142-164,195-219): with the k-NN distances r_ij of this shard,
 *   ell = log(sort(r)_ij) + log(pi) / 2   (n_local x k, 1 <= k <= 64, computed by the caller),
 *   dims = exp(mu_dim + L z[0]),  log_dens = mu_dens + L z[1],
 *   pred_ij = log_dens_i + dims_i ell_ij - lnGamma(dims_i / 2 + 1),
 *   loss(z) = 1/2 |z|^2 + log 2 pi - sum_ij [pred_ij j - exp(pred_ij) - lnGamma(j)]
 * (the prior's constant is the reference's (K/2) log 2 pi with K = 2 latent functions, dimensionality_estimator.py:389-394).
 * z, grad, hess_diag: 2 x m, row 0 the log-dimensionality, row 1 the log-density.  One pass over the n x m buffer per
 * evaluation computes both L z[0] and L z[1] and both back-projections; the Hessian diagonal (explicit L only, like
 * mln_objective) takes a second pass.  One pass covers m <= 5120 landmarks; beyond, MLN_ERR_UNSUPPORTED.  A non-finite
 * loss is returned as +inf.  Sums are all-reduced over ranks; prior terms are added once. */
int mln_fit_set_dim_likelihood(mln_fit* fit, const double* ell, int32_t k, double mu_dim, double mu_dens);
int mln_dim_objective(mln_fit* fit, const double* z, double* loss, double* grad /* 2 x m */,
                      double* hess_diag /* 2 x m or NULL */);

/* mln_dim_objective at S points in one call (the Monte-Carlo step of DimensionalityEstimator(optimizer="advi")):
 * loss[s], grad[s][:][:] = mln_dim_objective(fit, Z[s][:][:]) without the Hessian.  Z, grad: S x 2 x m row-major (sample s,
 * then row 0 the log-dimensionality, row 1 the log-density); loss: S.  Any S >= 1 (chunks of 32 samples inside: each
 * sample takes two columns of the skinny products, one per latent function).  Same likelihood
 * (mln_fit_set_dim_likelihood, hence the same 5120-landmark limit), same all-reduce over ranks (one per chunk: the
 * losses and the gradient block together), prior terms added once per sample; a non-finite loss is returned as +inf.
 * Two passes over the n x m buffer per chunk instead of one per sample: F = B [W0 | W1] with the Poisson likelihood in
 * the epilogue, then G = B^T [C0 | C1], on the fp64 matrix cores (csrc/dim_objective_batch.hip).  Every handle layout is
 * batched: explicit and implicit factors, Nystroem projections, mln_fit_from_L, the full GP.  Bit-reproducible from
 * call to call. */
int mln_dim_objective_batch(mln_fit* fit, const double* Z, int32_t S, double* loss /* S */, double* grad /* S x 2 x m */);

/* a-11: f = L z + mu on this shard (inference.py:51-69,341-354).                                */
int mln_transform(mln_fit* fit, const double* z, double mu, double* f_out /* n_local */);

/* a-12: predictor weights.
 *   sparse-Cholesky:  w = Lp^-T z                       conditional.py:818
 *   full:             w = Lp^-T Lp^-1 (y - mu)          conditional.py:263-264                 */
int mln_weights_cholesky(mln_fit* fit, const double* z, double* w /* m */);
int mln_weights_full(mln_fit* fit, const double* y, int64_t p, double mu, double* w /* m x p */);

/* a-12 (FunctionEstimator, scalar sigma): conditional.py:513-547 + _sparse_solve :57-66
 *   A = Lp^-1 cov(xu,x);  L_B = chol(A A^T / sigma^2 + I);
 *   W = Lp^-T L_B^-T L_B^-1 A (y - mu) / sigma^2          (m x p)
 * x, y are this rank's shard; A A^T and A y are all-reduced.                                   */
int mln_sparse_solve(mln_ctx* ctx, const mln_kernel_desc* cov, const double* x, int64_t n_local,
                     int32_t d, const double* xu, int64_t m, const double* y, int64_t p, double mu,
                     double sigma, double jitter, double* W /* m x p */);
/* Same solve, additionally returning the with_uncertainty state of the noisy landmark conditional
 * (conditional.py:571-577): Lp (m x m) and Cs = Lp L_B (m x m, lower), either may be NULL.          */
int mln_sparse_solve_factors(mln_ctx* ctx, const mln_kernel_desc* cov, const double* x, int64_t n_local,
                             int32_t d, const double* xu, int64_t m, const double* y, int64_t p, double mu,
                             double sigma, double jitter, double* W, double* Lp_out, double* Cs_out);

/* Noise models of the landmark conditional beyond one scalar (conditional.py:13-43,140-159,529-545):
 *   MLN_SIGMA_SCALAR      sigma[1]        the solve above
 *   MLN_SIGMA_PER_OUTPUT  sigma[p]        one noise level per output column ("per-gene" sigma, the vmap of
 *                                         conditional.py:529-545); A A^T and A (y - mu) are formed once; adjacent
 *                                         columns with equal sigma share one L_B, and beyond 32 such runs one
 *                                         eigendecomposition A A^T = U diag(lam) U^T serves every level:
 *                                         (A A^T / s^2 + I)^-1 = U diag(1 / (lam / s^2 + 1)) U^T
 *   MLN_SIGMA_PER_CELL    sigma[n_local]  element-wise standard deviation of this rank's cells
 *                                         (`sigma.shape == r.shape`, conditional.py:155-159):
 *                                         L_B L_B^T = A diag(1/sigma^2) A^T + I, c = L_B^-1 A ((y - mu) / sigma^2)   */
enum { MLN_SIGMA_SCALAR = 0, MLN_SIGMA_PER_OUTPUT = 1, MLN_SIGMA_PER_CELL = 2 };
int mln_sparse_solve_noise(mln_ctx* ctx, const mln_kernel_desc* cov, const double* x, int64_t n_local,
                           int32_t d, const double* xu, int64_t m, const double* y, int64_t p, double mu,
                           const double* sigma, int32_t sigma_kind, double jitter, double* W /* m x p */);

/* The same solve for 2-D targets given in CSR (an AnnData `.X`): y (n_local x p) is indptr[n_local + 1], indices[nnz],
 * data[nnz] with nnz = indptr[n_local] -- HOST arrays (a device pointer is MLN_ERR_ARG).  sigma_kind is MLN_SIGMA_SCALAR
 * (sigma[1]; Lp_out / Cs_out as in mln_sparse_solve_factors, either may be NULL) or MLN_SIGMA_PER_OUTPUT (sigma[p], no
 * factors); MLN_SIGMA_PER_CELL is MLN_ERR_ARG (that model takes a 1-D y).
 * Before anything is launched one host pass checks indptr[0] == 0, indptr non-decreasing, per row the indices strictly
 * increasing and inside [0, p), the data finite: a violation is MLN_ERR_ARG with a message naming the row.
 * No n x p array is formed: y - mu exists one row panel at a time (a byte budget: rows = budget / 8p, a multiple of 64, at
 * least 64), built in HBM from the CSR arrays and fed to the GEMM that forms A (y - mu); the panels accumulate in a fixed
 * order, so two calls return the same bits.  Everything after that product is the code of the dense entries.            */
int mln_sparse_solve_csr(mln_ctx* ctx, const mln_kernel_desc* cov, const double* x, int64_t n_local, int32_t d,
                         const double* xu, int64_t m, const int64_t* indptr, const int32_t* indices,
                         const double* data, int64_t p, double mu, const double* sigma, int32_t sigma_kind,
                         double jitter, double* W /* m x p */, double* Lp_out, double* Cs_out);

/* Full GP conditioned on p outputs with one noise level each (conditional.py:239-251; leverage :313-323,385-403;
 * HC3 residuals :330-333; variance weights :338-350) from ONE eigendecomposition K = U diag(lam) U^T of the n x n
 * kernel matrix: (K + (sigma_j^2 + jitter) I)^-1 = U diag(1 / (lam + sigma_j^2 + jitter)) U^T.
 * W: n x p.  leverage, corrected_r2, variance_W: n x p or NULL (each needs the one before it).                         */
int mln_full_conditional_noise(mln_ctx* ctx, const mln_kernel_desc* cov, const double* x, int64_t n, int32_t d,
                               const double* y, int64_t p, double mu, const double* sigma /* p */, double jitter,
                               double* W, double* leverage, double* corrected_r2, double* variance_W);

/* Leverage of the landmark conditional for p noise levels at once (conditional.py:660-685 applied per level by the
 * vmap of :672-680):  out[i][j] = b_i^T (sigma_j^2 K_uu + B^T B + jitter I)^-1 b_i  with B = cov(x, xu) over the cells
 * of all ranks, b_i the rows of this rank, and K_uu = Lk Lk^T given by its lower factor Lk (m x m; the predictor's L).
 * One eigendecomposition of L^T L + jitter Lk^-1 Lk^-T (L = B Lk^-T) serves every level.                              */
int mln_landmark_leverage(mln_ctx* ctx, const mln_kernel_desc* cov, const double* x, int64_t n_local, int32_t d,
                          const double* xu, int64_t m, const double* Lk, const double* sigma, int64_t p,
                          double jitter, double* out /* n_local x p */);

/* a-13: mean(Xnew) = mu + cov(Xnew, centers) W   (conditional.py:366-373,651-658,899-906).
 * centers: m x d (landmarks or, full GP, the training cells); W: m x p; out: n_new x p.
 * cov(Xnew, centers) is never materialised for p == 1.                                         */
int mln_predict_mean(mln_ctx* ctx, const mln_kernel_desc* cov, const double* xnew, int64_t n_new,
                     int32_t d, const double* centers, int64_t m, const double* W, int64_t p,
                     double mu, double* out);

/* ---- diagnostics: measured rooflines of this device and the GEMM kernel in isolation ----------
 *   mln_diag_peak   what = 0: fp64 MFMA issue peak (TFLOP/s); 1: HBM streaming read, 4: streaming write (GB/s)
 *   mln_diag_dgemm  milliseconds per call of C = op(A) op(B) (same arguments as the internal GEMM) */
int mln_diag_peak(mln_ctx* ctx, int32_t what, int64_t bytes, double* result);
int mln_diag_dgemm(mln_ctx* ctx, int32_t ta, int32_t tb, int64_t M, int64_t N, int64_t K,
                   int32_t lower_only, int32_t split_k, int32_t reps, double* ms_out);
/* The GEMM's mixed-tile pipelined kernel against its single-size kernels on the same pseudo-random operands
 * (alpha = 0.75, the given beta; lower_only 0..3 and kmode 0..7 as the internal GEMM takes them: whole matrix / a triangle of
 * tiles, full / block-diagonal / triangular K ranges -- decomposition.py:111-123,205-210 and conditional.py:57-66 reach
 * it in every one of them).  out[0] = largest absolute difference (0 expected: the same summation order per element),
 * out[1] = largest absolute value.  any_size != 0: the mixed kernel also below the size where the policy selects it. */
int mln_diag_dgemm_compare(mln_ctx* ctx, int32_t ta, int32_t tb, int64_t M, int64_t N, int64_t K, int32_t lower_only,
                           int32_t kmode, double beta, int32_t any_size, double* out);
/* One launch of the internal GEMM on caller-supplied host buffers, for tests that hold an exact expected result
 * (tests/gemm_reference.py).  The fields are those of the internal GEMM; in addition
 *   a_off, b_off, c_off  element offsets of the operands in their buffers (odd: 8- but not 16-byte aligned: scalar loads)
 *   bsa, bsb, bsc        batch > 1: distance in elements between consecutive operands (bsc >= split_k * M * ldc)
 *   mix                  0: the single-size tile kernels only; otherwise the launch policy's own choice
 *   sum_partials         split_k > 1 only: follow with the fixed-order sum of the partials, out = beta * out + sum
 *   c_in_a_col           >= 0: C lies INSIDE the A operand, at this element offset from its start, with ldc = lda
 *   c_in_b_off           >= 0: the same inside the B operand, ldc = ldb   (both -1: C is the third buffer)
 * split_k > 1: C holds split_k partial results M * ldc elements apart (alpha applied, beta not).  C is uploaded, and
 * downloaded whole; in place its count must equal that of the aliased buffer, whose final contents it receives.
 * MLN_ERR_ARG unless whole rows of every operand lie inside the given element counts. */
typedef struct mln_gemm_spec {
  int32_t ta, tb, lower_only, kmode, split_k, batch, mix, sum_partials;
  int64_t M, N, K, lda, ldb, ldc;
  int64_t a_off, b_off, c_off;
  int64_t bsa, bsb, bsc;
  int64_t c_in_a_col, c_in_b_off;
  double alpha, beta;
} mln_gemm_spec;
int mln_diag_dgemm_run(mln_ctx* ctx, const mln_gemm_spec* spec, const double* A, int64_t a_count, const double* B,
                       int64_t b_count, double* C, int64_t c_count, double* out /* M * ldc, or NULL */, int64_t out_count);
/* The integer Gram of the preconditioner in isolation (csrc/gram_i8.hip): out (m x m) = Q^T Q / 8355711^2 with
 * Q = round(A * 8355711), A rows x m with values in [0, 1] (host or device); terms below 2^-23 relative are dropped.
 * ms_out (may be NULL): milliseconds per call over `reps` calls.  Not a reference operation: the reference forms the
 * fp64 Gram of all cells (parameters.py:895-896); this one only ever feeds the preconditioner. */
int mln_diag_gram_i8(mln_ctx* ctx, const double* A, int64_t rows, int64_t m, double* out, int32_t reps, double* ms_out);
/* ms of: kernel-matrix pass alone, Gram GEMM alone, both on two streams, Cholesky alone, kernel matrix ||
 * Cholesky, kernel matrix || (Cholesky then Gram) -- the measurement behind the two-stream set-up phase. */
int mln_diag_overlap(mln_ctx* ctx, int64_t n, int64_t m, int32_t d, int64_t gram_rows, double* out /* 6 */);
/* The fp16-split row-minimum sweep for cells with 65 to 256 features (csrc/rowmin_wide.hip) in isolation: x (n x d) against
 * y (m x d), host or device, the pair (i, i + self_offset) skipped when exclude_self != 0.  Everything lives in the centred,
 * scaled units x' = (x - centre) * scale that prep describes: m1[i] / m2[i] the smallest and second-smallest approximate
 * value of s_ij = |y'_j|^2 - 2 x'_i . y'_j over j, arg[i] the column of the smallest, E[i] the bound on |approximate - exact|
 * that the certification of the exact 1-NN search allows row i.  Requires 65 <= d <= 256.        */
int mln_diag_rowmin_wide(mln_ctx* ctx, const double* x, int64_t n, const double* y, int64_t m, int32_t d,
                         int64_t self_offset, int32_t exclude_self, float* m1, float* m2, int32_t* arg, double* E,
                         double* prep /* d + 2: centre, scale, max centred squared norm */);
/* What this context's last mln_nn_distances did: out[0] the route (0 scalar exact, 1 fp64 matrix-core exact, 2 pre-filter
 * d <= 64, 3 pruned, 4 wide: 65 <= d <= 256), out[1] rows the certification left open, out[2] rows resolved by the exact
 * re-search, out[3] unused (0).                                                                  */
int mln_diag_nn_last(mln_ctx* ctx, double* out /* 4 */);
/* One launch of the fp64 objective kernel over `count` rows of the fit's buffer: first + i * stride (rows == NULL), or
 * rows[i] with optional per-row weights on the likelihood term.  Host pointers.  loss: the likelihood sum (times out_scale
 * when that is non-zero), grad (m): the rows' part of the gradient, f_rows (count): f of the rows in launch order; no prior. */
int mln_diag_objective_rows(mln_fit* fit, const double* z, int64_t count, int64_t first, int64_t stride,
                            const int64_t* rows, const double* row_w, double out_scale, double* loss, double* grad,
                            double* f_rows);

/* ---- predictive uncertainty (S8f rank 2) ----------------------------------------------------------
 * covariance:       k(x*,x*) - A A^T with A = cov(x*, centers) Lf^-T      conditional.py:409-422,930-945
 * mean covariance:  (K W)(K W)^T with K = cov(x*, centers), W m x q        conditional.py:423-440,947-963
 * diag != 0: out has n_new entries (the variances); diag == 0: out is n_new x n_new (n_new <= 32768). */
int mln_predict_covariance(mln_ctx* ctx, const mln_kernel_desc* cov, const double* xnew, int64_t n_new,
                           int32_t d, const double* centers, int64_t m, const double* Lf, int32_t diag,
                           double* out);
int mln_predict_mean_covariance(mln_ctx* ctx, const mln_kernel_desc* cov, const double* xnew, int64_t n_new,
                                int32_t d, const double* centers, int64_t m, const double* W, int64_t q,
                                int32_t diag, double* out);

/* Both variances for n queries at T times in one call, for cov((x,t),(c,s)) = k_state(x,c) k_time(t,s).
 * state: the state factor's program over all d columns; S (T x m) = k_time(t, s_j), kdiag (T) = k_time(t, t), from the
 * caller.  cov_out / mcov_out: n x T row-major, either may be NULL (not both):
 *   cov [i,t] = kss_i kdiag_t - |K_t Lf^-T|^2  (+ |K_t Cs^-T|^2 with Cs, as the noisy landmark conditional adds it)
 *   mcov[i,t] = |K_t W|^2 for W (m x q), or sum_q w_std_q^2 (K_t Lf^-T)_q^2 for w_std (m) -- W = Lf^-T diag(w_std) without a
 *   second product; W and w_std exclude each other.
 * scratch_doubles: the budget of the row-chunk and time-block buffers (0: 2^27); never fewer than 64 rows or one time. */
int mln_predict_variance_grid(mln_ctx* ctx, const mln_kernel_desc* state, const double* xq, int64_t n, int32_t d,
                              const double* centers, int64_t m, const double* S, int64_t T, const double* kdiag,
                              const double* Lf, const double* Cs, const double* W, int64_t q, const double* w_std,
                              int64_t scratch_doubles, double* cov_out, double* mcov_out);

/* wall-clock seconds of the stages of the last mln_fit_prepare / mln_ridge_init and counters
 * of mln_objective: [0] kernel matrix, [1] cholesky, [2] trsm, [3] ridge gram, [4] ridge solve,
 * [5] objective kernel time (sum, HIP events), [6] objective launches, [7] bytes of L streamed
 * per objective launch; [8] / [9] the same time / launch count for the warm-up passes of mln_map_solve on the
 * 32-bit copy (mixed precision: they stream 4 bytes per element, half of [7]); [10] the format of that copy:
 * 0 none, 1 fp32 values, 2 32-bit fixed point round(v 2^32) (covariances bounded by 1); [11] seconds spent on
 * other ranks' column blocks under MELLON_AMD_EMULATE_RANKS (tools/emulate_rank.py; 0 otherwise), already excluded
 * from [3] and [4].
 * [12] / [13] kernel seconds / launches of the solver's subsample passes (every [14]-th row: the cells of the preconditioner's
 * Gram); [15] wall seconds and [16] count of preconditioner rebuilds inside mln_map_solve; [17] passes over the n x m buffer in
 * full-fp64-pass equivalents ([6] + [9] / 2 + [13] / [14]); [18] rebuilds that declined (the sample's weights span more
 * than 1e5) or lost positive definiteness -- the solve went on with the first preconditioner; [19] rebuilt preconditioners
 * that failed their trial (no convergence within 60 iterations) and were replaced by the first again; [20] halvings of a
 * start whose loss was not finite or above 1e30; [21] how the last mln_fit_gram_rank counted: 1 = inertia of G - x I
 * (csrc/ldl_inertia.hip), 2 = tridiagonalisation + Sturm counts (csrc/tridiag.hip), 0 = not called; importance tail of
 * mln_map_solve (passes over an importance-sampled row list after the rebuild): [22] launches -- not in [6], counted in [17]
 * by rows / n --, [23] rows of this rank's list, [24] kernel seconds, [25] times its guard fired (the full loss rose: the
 * solve went back to the last anchor and finished on full passes).                                                        */
#define MLN_N_STAGE_TIMES 26
int mln_stage_times(mln_fit* fit, double* out /* MLN_N_STAGE_TIMES */);

#ifdef __cplusplus
}
#endif
#endif /* MELLON_HIP_H */
