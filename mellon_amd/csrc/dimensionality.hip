// Local intrinsic dimensionality: the exact k-nearest-neighbour search, the per-cell fractal dimension and the MAP objective
// of the dimensionality / density pair (reference mellon/dimensionality_estimator.py, util.py:486-536, inference.py:95-219).
//
//   k_knn            exact k-NN, one workgroup per 64 queries: candidates stream through LDS in tiles of 64 rows and 16
//                    features; a 4 x 4 register block per thread accumulates squared differences (difference form, fp64:
//                    the reported distances are sqrt(sum (x - y)^2) of these very sums); pairs at or below the query's
//                    current k-th distance go to a per-query LDS buffer, which one wave merges into the query's sorted
//                    list (ties: smaller index first).  O(n k) working memory, no n x m buffer.
//   k_local_dim      one workgroup per query: the k(k-1)/2 pair distances of its neighbourhood (features tiled through LDS),
//                    a bitonic sort in LDS, the closed-form least-squares slope of log(1..kc2) on log(distance).
//   k_dim_objective  one pass over the n x m buffer per evaluation: both L z0 and L z1 from the same loaded rows, the k
//                    Poisson terms of each row, both back-projections (and the Hessian diagonals) from the same registers.
//                    A sibling of k_objective (objective.hip): same workgroup shape, same contiguous per-workgroup row ranges,
//                    same fixed-order reduction (k_reduce_obj) -- deterministic.
#include "api_internal.h"
#include "dim_gamma.h"

namespace {

// ---- exact k-NN -------------------------------------------------------------------------------------------
constexpr int KNN_WG = 256;
constexpr int KNN_QB = 64;     // queries per workgroup
constexpr int KNN_CB = 64;     // candidates per tile
constexpr int KNN_DC = 16;     // features per LDS stage
constexpr int KNN_KMAX = 64;

struct KnnArgs {
  const double* x; int64_t n;
  const double* y; int64_t m;
  int d, k;
  int exclude; int64_t self_offset;
  double* dist; int64_t* idx;
};

__global__ __launch_bounds__(KNN_WG) void k_knn(KnnArgs a) {
  __shared__ double qs[KNN_DC][KNN_QB];
  __shared__ double cs[KNN_DC][KNN_CB];
  __shared__ double topd[KNN_QB][KNN_KMAX];
  __shared__ int topi[KNN_QB][KNN_KMAX];
  __shared__ double cand_d[KNN_QB][KNN_CB];
  __shared__ int cand_i[KNN_QB][KNN_CB];
  __shared__ int cnt[KNN_QB];
  __shared__ double thr[KNN_QB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tq = tid >> 4, tc = tid & 15;          // queries 4 tq .. 4 tq + 3, candidates tc + 16 c
  const int64_t q0 = (int64_t)blockIdx.x * KNN_QB;
  const int k = a.k;
  for (int i = tid; i < KNN_QB * KNN_KMAX; i += KNN_WG) {
    topd[i / KNN_KMAX][i % KNN_KMAX] = __builtin_inf();
    topi[i / KNN_KMAX][i % KNN_KMAX] = 0x7fffffff;
  }
  if (tid < KNN_QB) { thr[tid] = __builtin_inf(); cnt[tid] = 0; }
  __syncthreads();
  for (int64_t c0 = 0; c0 < a.m; c0 += KNN_CB) {
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    for (int f0 = 0; f0 < a.d; f0 += KNN_DC) {
      // stage 64 query rows and 64 candidate rows x 16 features (zero beyond d; rows past the end repeat the last row)
      for (int i = tid; i < KNN_QB * KNN_DC; i += KNN_WG) {
        const int r = i / KNN_DC, f = i % KNN_DC;
        const int64_t qr = (q0 + r < a.n) ? q0 + r : a.n - 1;
        const int64_t cr = (c0 + r < a.m) ? c0 + r : a.m - 1;
        const bool fok = f0 + f < a.d;
        qs[f][r] = fok ? a.x[qr * a.d + f0 + f] : 0.0;
        cs[f][r] = fok ? a.y[cr * a.d + f0 + f] : 0.0;
      }
      __syncthreads();
#pragma unroll 4
      for (int f = 0; f < KNN_DC; ++f) {
        double qv[4], cv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) qv[i] = qs[f][4 * tq + i];
#pragma unroll
        for (int j = 0; j < 4; ++j) cv[j] = cs[f][tc + 16 * j];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const double df = qv[i] - cv[j];
            acc[i][j] = fma(df, df, acc[i][j]);
          }
      }
      __syncthreads();
    }
    // screen against the k-th distance so far; survivors go to the query's buffer (at most KNN_CB per tile)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ql = 4 * tq + i;
      const int64_t qi = q0 + ql;
      const double t = thr[ql];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t cj = c0 + tc + 16 * j;
        const bool ok = qi < a.n && cj < a.m && !(a.exclude && cj == qi + a.self_offset) && acc[i][j] <= t;
        if (ok) {
          const int s = atomicAdd(&cnt[ql], 1);
          cand_d[ql][s] = acc[i][j];
          cand_i[ql][s] = (int)cj;
        }
      }
    }
    __syncthreads();
    // merge: wave w takes queries w, w + 4, ...; lane l holds entry l of the sorted list
    for (int ql = wave; ql < KNN_QB; ql += KNN_WG / 64) {
      const int c = cnt[ql];
      if (c == 0) continue;
      double ld = topd[ql][lane];
      int li = topi[ql][lane];
      for (int s = 0; s < c; ++s) {
        const double cd = cand_d[ql][s];
        const int ci = cand_i[ql][s];
        const bool less = lane < k && (ld < cd || (ld == cd && li < ci));
        const int pos = __popcll(__ballot(less));
        const double upd = __shfl_up(ld, 1, 64);
        const int upi = __shfl_up(li, 1, 64);
        if (pos < k) {
          if (lane == pos) { ld = cd; li = ci; }
          else if (lane > pos) { ld = upd; li = upi; }
        }
      }
      topd[ql][lane] = ld;
      topi[ql][lane] = li;
      if (lane == k - 1) thr[ql] = ld;
      if (lane == 0) cnt[ql] = 0;
    }
    __syncthreads();
  }
  // out: sqrt of the difference-form sums, ascending
  for (int i = tid; i < KNN_QB * k; i += KNN_WG) {
    const int ql = i / k, j = i % k;
    const int64_t qi = q0 + ql;
    if (qi >= a.n) continue;
    const double dd = topd[ql][j];
    a.dist[qi * k + j] = sqrt(dd);
    if (a.idx) a.idx[qi * k + j] = (topi[ql][j] == 0x7fffffff) ? -1 : (int64_t)topi[ql][j];
  }
}

// ---- local fractal dimension -------------------------------------------------------------------------------
constexpr int LD_WG = 256;
constexpr int LD_DC = 32;
constexpr int LD_KMAX = 64;
constexpr int LD_PMAX = 2048;                    // >= 64 * 63 / 2 = 2016, a power of two for the bitonic sort
constexpr int LD_PPT = LD_PMAX / LD_WG;          // pairs per thread

__device__ __forceinline__ double block_sum_ld(double v, double* red) {
  // fixed-order sum over the workgroup: butterfly in each wave, then the four wave totals in order
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(LD_WG) void k_local_dim(const double* __restrict__ x, int64_t n, int d,
                                                     const int64_t* __restrict__ nbr, int k, double* __restrict__ out) {
  __shared__ double xs[LD_KMAX][LD_DC + 1];
  __shared__ double sd[LD_PMAX];
  __shared__ int64_t rows[LD_KMAX];
  __shared__ unsigned char pa[LD_PMAX], pb[LD_PMAX];
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const int64_t q = blockIdx.x;
  const int kc2 = k * (k - 1) / 2;
  if (tid < k) {
    int64_t r = nbr[q * k + tid];
    rows[tid] = r < 0 ? 0 : (r >= n ? n - 1 : r);      // (the host validates; a bad index must not read out of bounds)
    const int off = tid * (2 * k - tid - 1) / 2;        // pairs (tid, j), j > tid, in row-major triangle order
    for (int j = tid + 1; j < k; ++j) { pa[off + j - tid - 1] = (unsigned char)tid; pb[off + j - tid - 1] = (unsigned char)j; }
  }
  __syncthreads();
  double acc[LD_PPT];
#pragma unroll
  for (int t = 0; t < LD_PPT; ++t) acc[t] = 0.0;
  for (int f0 = 0; f0 < d; f0 += LD_DC) {
    for (int i = tid; i < k * LD_DC; i += LD_WG) {
      const int r = i / LD_DC, f = i % LD_DC;
      xs[r][f] = (f0 + f < d) ? x[rows[r] * d + f0 + f] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < LD_PPT; ++t) {
      const int p = tid + t * LD_WG;
      if (p < kc2) {
        const int i = pa[p], j = pb[p];
        double s = acc[t];
        for (int f = 0; f < LD_DC; ++f) {
          const double df = xs[i][f] - xs[j][f];
          s = fma(df, df, s);
        }
        acc[t] = s;
      }
    }
    __syncthreads();
  }
  int ns = 2;
  while (ns < kc2) ns <<= 1;
#pragma unroll
  for (int t = 0; t < LD_PPT; ++t) {
    const int p = tid + t * LD_WG;
    if (p < ns) sd[p] = (p < kc2) ? sqrt(acc[t]) : __builtin_inf();
  }
  __syncthreads();
  // bitonic sort of sd[0, ns), ascending
  for (int size = 2; size <= ns; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < ns / 2; t += LD_WG) {
        const int lo = 2 * t - (t & (stride - 1));
        const int hi = lo + stride;
        const bool up = (lo & size) == 0;
        const double u = sd[lo], v = sd[hi];
        if ((u > v) == up) { sd[lo] = v; sd[hi] = u; }
      }
      __syncthreads();
    }
  }
  // slope of y = log(1..kc2) on A = [a, 1], a = log(distance), as lstsq returns it: the closed form
  // sum (a - abar)(y - ybar) / sum (a - abar)^2 while A has full rank, the minimum-norm solution once it has rank 1
  double sa = 0.0, sy = 0.0;
  for (int p = tid; p < kc2; p += LD_WG) { sa += log(sd[p]); sy += log((double)(p + 1)); }
  const double abar = block_sum_ld(sa, red) / kc2;
  const double ybar = block_sum_ld(sy, red) / kc2;
  double sxy = 0.0, sxx = 0.0;
  for (int p = tid; p < kc2; p += LD_WG) {
    const double da = log(sd[p]) - abar, dy = log((double)(p + 1)) - ybar;
    sxy = fma(da, dy, sxy);
    sxx = fma(da, da, sxx);
  }
  const double Sxy = block_sum_ld(sxy, red);
  const double Sxx = block_sum_ld(sxx, red);
  if (tid == 0) {
    // A^T A = [[p, qq], [qq, N]], p = sum a^2, qq = sum a, det = N Sxx; eigenvalues (p + N) / 2 +- disc.  lstsq's rank
    // rule: s_min <= eps max(N, 2) s_max, i.e. det <= (tol lam1)^2.  Rank 1 (an equidistant neighbourhood, to rounding;
    // always for k = 2): slope = v1[0] (v1 . A^T y) / lam1, v1 the top eigenvector, from whichever of its two closed
    // forms has no cancellation.  A zero distance gives NaN, like the reference's lstsq.
    const double N = (double)kc2;
    const double p = fma(N * abar, abar, Sxx), qq = N * abar;
    const double det = N * Sxx;
    const double h = 0.5 * (p - N), disc = sqrt(fma(h, h, qq * qq));
    const double lam1 = 0.5 * (p + N) + disc;
    const double tol = __DBL_EPSILON__ * (kc2 > 2 ? N : 2.0) * lam1;
    double r;
    if (!isfinite(abar)) {
      r = __builtin_nan("");
    } else if (det > tol * tol) {
      r = Sxy / Sxx;
    } else {
      const double v0 = h >= 0.0 ? disc + h : qq, v1 = h >= 0.0 ? qq : disc - h;
      const double aty0 = fma(N * abar, ybar, Sxy), aty1 = N * ybar;   // A^T y = [sum a y, sum y]
      r = v0 * fma(v0, aty0, v1 * aty1) / (fma(v0, v0, v1 * v1) * lam1);
    }
    out[q] = r;
  }
}

// ---- dimensionality objective --------------------------------------------------------------------------------
constexpr int DWG = 512;
typedef double d2 __attribute__((ext_vector_type(2)));

struct DimArgs {
  const double* L; int64_t ldl; int64_t n; int64_t m;
  const double* z;        // 2 x ldl: z0 (log-dimensionality), z1 (log-density); w = Lp^-T z in implicit mode
  const double* ell;      // n x k: log(sorted distance) + log(pi) / 2
  int k;
  double mu_dim, mu_dens;
  double* part;           // n_wg x 4 ldl: g0 | g1 | h0 | h1
  double* part_loss;      // n_wg
  int n_wg;
};

template <int CPT, int R>
__device__ __forceinline__ void dim_load_rows(const d2* __restrict__ L2, int64_t ld2, int64_t row, int64_t n, int tid,
                                              d2 (&v)[R][CPT]) {
  // unconditional, clamped loads (see objective.hip load_rows): rows past the end re-read the step's first row
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const d2* rowp = L2 + ((row + r) < n ? (row + r) : row) * ld2;
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      unsigned off = (unsigned)c * DWG + tid;
      off = off < (unsigned)ld2 ? off : (unsigned)ld2 - 1u;
      v[r][c] = __builtin_nontemporal_load(rowp + off);
    }
  }
}

// this lane's distance terms of the step: term t = lane + 64 it is (row t / k, neighbour t % k)
template <int R>
__device__ __forceinline__ void dim_load_ell(const DimArgs& a, int64_t row, const int (&tr)[R], const int (&tj)[R],
                                             const bool (&tv)[R], double (&e)[R]) {
#pragma unroll
  for (int it = 0; it < R; ++it) {
    const int64_t i = (row + tr[it] < a.n) ? row + tr[it] : a.n - 1;
    e[it] = tv[it] ? a.ell[i * a.k + tj[it]] : 0.0;
  }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <int CPT, int R, bool HESS>
__device__ __forceinline__ void dim_process(const DimArgs& a, int64_t row, int tid, int par, const d2 (&v)[R][CPT],
                                            const d2 (&z0)[CPT], const d2 (&z1)[CPT], d2 (&g0)[CPT], d2 (&g1)[CPT],
                                            double& loss, double (*red)[8][2 * R],
                                            const double* lgj, const int (&tr)[R], const int (&tj)[R],
                                            const bool (&tv)[R], const double (&ell)[R]) {
  const int wave = tid >> 6, lane = tid & 63;
  double dot[2 * R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      s0 = fma(v[r][c].x, z0[c].x, s0);
      s0 = fma(v[r][c].y, z0[c].y, s0);
      s1 = fma(v[r][c].x, z1[c].x, s1);
      s1 = fma(v[r][c].y, z1[c].y, s1);
    }
    dot[2 * r] = wave_sum(s0);
    dot[2 * r + 1] = wave_sum(s1);
  }
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < 2 * R; ++q) red[par][wave][q] = dot[q];
  }
  __syncthreads();
  double f0[R], f1[R], D[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int w = 0; w < 8; ++w) { s0 += red[par][w][2 * r]; s1 += red[par][w][2 * r + 1]; }
    f0[r] = s0;
    f1[r] = s1;
    D[r] = exp(a.mu_dim + s0);                 // inference.py:160-162: dims = exp(mu_dim + L z0)
  }
  // per-row constants once per step, lane r < R for row r: lnGamma(D / 2 + 1), psi(D / 2 + 1) (and psi'), then fetched by
  // the lanes that hold that row's terms
  const int rl = lane < R ? lane : 0;
  double Dl = D[0];
#pragma unroll
  for (int rr = 1; rr < R; ++rr) if (rl == rr) Dl = D[rr];
  const double xh = 0.5 * Dl + 1.0;
  double lg_own, ps_own, tp_own;
  gamma_fns<HESS>(xh, lg_own, ps_own, tp_own);
  // the Poisson terms (inference.py:112-120), one per lane: pred = log_dens + D ell - lgamma(D / 2 + 1)
  double sa[R], sas[R], se[R], sh[R], sl[R];
#pragma unroll
  for (int r = 0; r < R; ++r) sa[r] = sas[r] = se[r] = sh[r] = sl[r] = 0.0;
#pragma unroll
  for (int it = 0; it < R; ++it) {
    const int r = tr[it];
    double fd = f1[0], Dr = D[0];
#pragma unroll
    for (int rr = 1; rr < R; ++rr) if (r == rr) { fd = f1[rr]; Dr = D[rr]; }
    const bool ok = tv[it] && (row + r) < a.n;
    const double lg = __shfl(lg_own, r, 64), ps = __shfl(ps_own, r, 64);
    const double pred = (a.mu_dens + fd) + Dr * ell[it] - lg;
    const double e = exp(pred);
    const double cntj = (double)(tj[it] + 1);
    const double av = cntj - e;
    const double s = ell[it] - 0.5 * ps;
    const double qa = ok ? av : 0.0, qas = ok ? av * s : 0.0, qe = ok ? e : 0.0;
    const double ql = ok ? fma(pred, cntj, -e) - lgj[tj[it]] : 0.0;
    double qh = 0.0;
    if (HESS) qh = ok ? fma(e * s, s, 0.25 * av * __shfl(tp_own, r, 64)) : 0.0;
#pragma unroll
    for (int rr = 0; rr < R; ++rr) {
      const bool mine = r == rr;
      sa[rr] += mine ? qa : 0.0;
      sas[rr] += mine ? qas : 0.0;
      se[rr] += mine ? qe : 0.0;
      sl[rr] += mine ? ql : 0.0;
      if (HESS) sh[rr] += mine ? qh : 0.0;
    }
  }
  // gradient pass: c0 = d loss / d (L z0)_i, c1 = d loss / d log_dens_i, accumulated as c row;
  // Hessian pass: the second derivatives, accumulated as c row^2 (same registers: a separate pass, see mln_dim_objective)
  double c0[R], c1[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const bool rok = (row + r) < a.n;
    const double Sas = wave_sum(sas[r]);
    if (HESS) {
      const double Se = wave_sum(se[r]), Sh = wave_sum(sh[r]);
      c1[r] = rok ? Se : 0.0;
      c0[r] = rok ? fma(D[r] * D[r], Sh, -D[r] * Sas) : 0.0;
    } else {
      const double Sa = wave_sum(sa[r]), Sl = wave_sum(sl[r]);
      c1[r] = rok ? -Sa : 0.0;
      c0[r] = rok ? -D[r] * Sas : 0.0;
      if (tid == 0 && rok) loss -= Sl;
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      const double w0x = HESS ? c0[r] * v[r][c].x : c0[r], w0y = HESS ? c0[r] * v[r][c].y : c0[r];
      const double w1x = HESS ? c1[r] * v[r][c].x : c1[r], w1y = HESS ? c1[r] * v[r][c].y : c1[r];
      g0[c].x = fma(w0x, v[r][c].x, g0[c].x);
      g0[c].y = fma(w0y, v[r][c].y, g0[c].y);
      g1[c].x = fma(w1x, v[r][c].x, g1[c].x);
      g1[c].y = fma(w1y, v[r][c].y, g1[c].y);
    }
  }
}

template <int CPT, int R, bool HESS>
__global__ __launch_bounds__(DWG) void k_dim_objective(DimArgs a) {
  __shared__ double red[2][8][2 * R];
  __shared__ double lgj[64];
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < 64) lgj[tid] = lgamma((double)(tid + 1));   // lnGamma(j), j = 1 .. 64
  const int64_t ld2 = a.ldl / 2;
  const d2* __restrict__ L2 = reinterpret_cast<const d2*>(a.L);
  const int64_t nsteps = (a.n + R - 1) / R;
  const int64_t per = (nsteps + a.n_wg - 1) / a.n_wg;
  const int64_t s_beg = (int64_t)blockIdx.x * per;
  int64_t s_end = s_beg + per;
  if (s_end > nsteps) s_end = nsteps;
  d2 z0[CPT], z1[CPT], g0[CPT], g1[CPT];
#pragma unroll
  for (int c = 0; c < CPT; ++c) {
    const int64_t col = 2 * ((int64_t)c * DWG + tid);
    z0[c] = z1[c] = g0[c] = g1[c] = (d2){0.0, 0.0};
    if (col < a.m) { z0[c].x = a.z[col]; z1[c].x = a.z[a.ldl + col]; }
    if (col + 1 < a.m) { z0[c].y = a.z[col + 1]; z1[c].y = a.z[a.ldl + col + 1]; }
  }
  int tr[R], tj[R];
  bool tv[R];
#pragma unroll
  for (int it = 0; it < R; ++it) {
    const int t = lane + 64 * it;
    tv[it] = t < R * a.k;
    tr[it] = tv[it] ? t / a.k : 0;
    tj[it] = tv[it] ? t % a.k : 0;
  }
  __syncthreads();
  double loss = 0.0;
  d2 va[R][CPT], vb[R][CPT];
  double ea[R], eb[R];
  const int64_t s_last = s_end - 1;
  if (s_beg < s_end) { dim_load_rows<CPT, R>(L2, ld2, s_beg * R, a.n, tid, va); dim_load_ell<R>(a, s_beg * R, tr, tj, tv, ea); }
  for (int64_t s = s_beg; s < s_end; s += 2) {
    const int64_t s1 = (s + 1 < s_end) ? s + 1 : s_last, s2 = (s + 2 < s_end) ? s + 2 : s_last;
    dim_load_rows<CPT, R>(L2, ld2, s1 * R, a.n, tid, vb);
    dim_load_ell<R>(a, s1 * R, tr, tj, tv, eb);
    dim_process<CPT, R, HESS>(a, s * R, tid, 0, va, z0, z1, g0, g1, loss, red, lgj, tr, tj, tv, ea);
    dim_load_rows<CPT, R>(L2, ld2, s2 * R, a.n, tid, va);
    dim_load_ell<R>(a, s2 * R, tr, tj, tv, ea);
    if (s + 1 < s_end) dim_process<CPT, R, HESS>(a, (s + 1) * R, tid, 1, vb, z0, z1, g0, g1, loss, red, lgj, tr, tj, tv, eb);
  }
  double* pg = a.part + (int64_t)blockIdx.x * 4 * a.ldl + (HESS ? 2 * a.ldl : 0);
#pragma unroll
  for (int c = 0; c < CPT; ++c) {
    const int64_t col = 2 * ((int64_t)c * DWG + tid);
    if (col < a.ldl) {
      *reinterpret_cast<d2*>(pg + col) = g0[c];
      *reinterpret_cast<d2*>(pg + a.ldl + col) = g1[c];
    }
  }
  if (tid == 0 && !HESS) a.part_loss[blockIdx.x] = loss;
}

template <int CPT, int R>
int launch_dim_cpt(mln_ctx* ctx, const DimArgs& a, bool hess) {
  if (hess) hipLaunchKernelGGL((k_dim_objective<CPT, R, true>), dim3((unsigned)a.n_wg), dim3(DWG), 0, ctx->stream, a);
  else hipLaunchKernelGGL((k_dim_objective<CPT, R, false>), dim3((unsigned)a.n_wg), dim3(DWG), 0, ctx->stream, a);
  MLN_HIP(ctx, hipGetLastError());
  return MLN_OK;
}

// rows per step: two while the registers allow (four or five column pairs per thread leave room for one)
int launch_dim_objective(mln_ctx* ctx, const DimArgs& a, bool hess) {
  const int cpt = (int)((a.ldl / 2 + DWG - 1) / DWG);
  switch (cpt) {
    case 1: return launch_dim_cpt<1, 2>(ctx, a, hess);
    case 2: return launch_dim_cpt<2, 2>(ctx, a, hess);
    case 3: return launch_dim_cpt<3, 2>(ctx, a, hess);
    case 4: return launch_dim_cpt<4, 1>(ctx, a, hess);
    case 5: return launch_dim_cpt<5, 1>(ctx, a, hess);
    default: return MLN_ERR_UNSUPPORTED;
  }
}

constexpr int64_t DIM_MAX_LD = 5 * 2 * DWG;   // 5120 columns: five column pairs per thread

}  // namespace

// ---- C ABI ---------------------------------------------------------------------------------------------------

extern "C" int mln_knn(mln_ctx* ctx, const double* x, int64_t n, const double* y, int64_t m, int32_t d, int32_t k,
                       int32_t exclude, int64_t self_offset, double* dist, int64_t* idx) {
  if (!ctx) return MLN_ERR_ARG;
  if (n < 0 || m < 0 || d < 1) { mln_set_error(ctx, "knn: bad shape"); return MLN_ERR_SHAPE; }
  if (k < 1 || k > KNN_KMAX) { mln_set_error(ctx, "knn: k must lie in [1, 64]"); return MLN_ERR_SHAPE; }
  if (m >= 0x7fffffff) { mln_set_error(ctx, "knn: more than 2^31 - 1 candidate rows"); return MLN_ERR_SHAPE; }
  if (k > m - (exclude ? 1 : 0)) { mln_set_error(ctx, "knn: k exceeds the number of candidate rows"); return MLN_ERR_SHAPE; }
  if (n == 0) return MLN_OK;
  if (!x || !y || !dist) return MLN_ERR_ARG;
  MLN_HIP(ctx, hipSetDevice(ctx->device));
  DevIn dx, dy;
  DevOut o;
  MLN_TRY(dx.init(ctx, x, (size_t)n * d));
  if (y == x && m == n) dy.dev = dx.dev, dy.ctx = ctx; else MLN_TRY(dy.init(ctx, y, (size_t)m * d));
  MLN_TRY(o.init(ctx, dist, (size_t)n * k));
  int64_t* di = nullptr;
  DevBuf<int64_t> si;
  if (idx) {
    if (is_device_ptr(idx)) di = idx;
    else { MLN_TRY(si.alloc(ctx, (size_t)n * k, "neighbour indices")); di = si; }
  }
  KnnArgs a{dx.dev, n, dy.dev, m, d, k, exclude ? 1 : 0, self_offset, o.dev, di};
  hipLaunchKernelGGL(k_knn, dim3((unsigned)((n + KNN_QB - 1) / KNN_QB)), dim3(KNN_WG), 0, ctx->stream, a);
  MLN_HIP(ctx, hipGetLastError());
  if (idx && di != idx)
    MLN_HIP(ctx, hipMemcpyAsync(idx, di, sizeof(int64_t) * (size_t)n * k, hipMemcpyDeviceToHost, ctx->stream));
  return o.commit();   // (drains the stream: the index copy is idle when it is released)
}

extern "C" int mln_local_dimensionality(mln_ctx* ctx, const double* x, int64_t n, int32_t d, const int64_t* nbr,
                                        int64_t q, int32_t k, double* out) {
  if (!ctx) return MLN_ERR_ARG;
  if (n < 1 || q < 0 || d < 1) { mln_set_error(ctx, "local_dimensionality: bad shape"); return MLN_ERR_SHAPE; }
  if (k < 2 || k > LD_KMAX) { mln_set_error(ctx, "local_dimensionality: k must lie in [2, 64]"); return MLN_ERR_SHAPE; }
  if (q == 0) return MLN_OK;
  if (!x || !nbr || !out) return MLN_ERR_ARG;
  MLN_HIP(ctx, hipSetDevice(ctx->device));
  DevIn dx;
  DevOut o;
  MLN_TRY(dx.init(ctx, x, (size_t)n * d));
  MLN_TRY(o.init(ctx, out, (size_t)q));
  const int64_t* dn = nbr;
  DevBuf<int64_t> sn;
  if (!is_device_ptr(nbr)) {
    MLN_TRY(sn.alloc(ctx, (size_t)q * k, "neighbour indices"));
    MLN_HIP(ctx, hipMemcpyAsync(sn, nbr, sizeof(int64_t) * (size_t)q * k, hipMemcpyHostToDevice, ctx->stream));
    dn = sn;
  }
  hipLaunchKernelGGL(k_local_dim, dim3((unsigned)q), dim3(LD_WG), 0, ctx->stream, dx.dev, n, (int)d, dn, (int)k, o.dev);
  MLN_HIP(ctx, hipGetLastError());
  return o.commit();   // (drains the stream: the index copy is idle when it is released)
}

static int dim_one_pass_ok(mln_fit* f) {
  if (f->ldl > DIM_MAX_LD) {
    mln_set_error(f->ctx, "dimensionality objective: one pass covers at most " + std::to_string(DIM_MAX_LD) +
                              " columns of L (this fit has " + std::to_string(f->m) + ")");
    return MLN_ERR_UNSUPPORTED;
  }
  return MLN_OK;
}

extern "C" int mln_fit_set_dim_likelihood(mln_fit* f, const double* ell, int32_t k, double mu_dim, double mu_dens) {
  if (!f || (f->n > 0 && !ell)) return MLN_ERR_ARG;
  mln_ctx* ctx = f->ctx;
  if (k < 1 || k > 64) { mln_set_error(ctx, "set_dim_likelihood: k must lie in [1, 64]"); return MLN_ERR_SHAPE; }
  MLN_TRY(dim_one_pass_ok(f));
  MLN_HIP(ctx, hipSetDevice(ctx->device));
  const size_t ld = (size_t)f->ldl;
  if (f->dim_ell && f->dim_k != k) { (void)hipStreamSynchronize(ctx->stream); f->dim_ell.reset(); }
  if (!f->dim_ell) MLN_TRY(f->dim_ell.alloc(ctx, (size_t)(f->n > 0 ? f->n : 1) * k, "dim_ell"));
  if (!f->dim_part) MLN_TRY(f->dim_part.alloc(ctx, 4 * ld * (size_t)f->n_wg_cap, "dim_part"));
  if (!f->dim_z) {
    MLN_TRY(f->dim_z.alloc_zeroed(ctx, 4 * ld, "dim_z"));   // z (2 ld) and w (2 ld)
  }
  if (!f->dim_out) MLN_TRY(f->dim_out.alloc(ctx, (2 + 4 * ld), "dim_out"));
  if (f->n > 0)
    MLN_HIP(ctx, hipMemcpyAsync(f->dim_ell, ell, sizeof(double) * (size_t)f->n * k, hipMemcpyDefault, ctx->stream));
  MLN_HIP(ctx, hipStreamSynchronize(ctx->stream));
  f->dim_k = k;
  f->mu_dim = mu_dim;
  f->mu_dens = mu_dens;
  return MLN_OK;
}

extern "C" int mln_dim_objective(mln_fit* f, const double* z, double* loss, double* grad, double* hess_diag) {
  if (!f || !z || !loss || !grad) return MLN_ERR_ARG;
  mln_ctx* ctx = f->ctx;
  if (!f->dim_ell) { mln_set_error(ctx, "mln_fit_set_dim_likelihood has not been called"); return MLN_ERR_ARG; }
  if (hess_diag && f->kspace) {
    mln_set_error(ctx, "the Hessian diagonal needs the explicit factor L: prepare the fit without MLN_FIT_IMPLICIT");
    return MLN_ERR_UNSUPPORTED;
  }
  MLN_TRY(dim_one_pass_ok(f));
  MLN_HIP(ctx, hipSetDevice(ctx->device));
  MLN_TRY(fit_ensure_lp(f));
  const int64_t m = f->m, ld = f->ldl;
  std::vector<double> zh((size_t)(2 * m));
  MLN_HIP(ctx, hipMemcpyAsync(zh.data(), z, sizeof(double) * 2 * m, hipMemcpyDefault, ctx->stream));
  MLN_HIP(ctx, hipMemcpyAsync(f->dim_z, z, sizeof(double) * m, hipMemcpyDefault, ctx->stream));
  MLN_HIP(ctx, hipMemcpyAsync(f->dim_z + ld, z + m, sizeof(double) * m, hipMemcpyDefault, ctx->stream));
  DimArgs a{};
  a.L = f->L; a.ldl = ld; a.n = f->n; a.m = m;
  a.z = f->dim_z;
  if (f->kspace) {   // L z = K (Lp^-T z): both vectors through the triangular solve, the pass streams K
    double* w = f->dim_z + 2 * ld;
    MLN_HIP(ctx, hipMemcpyAsync(w, f->dim_z, sizeof(double) * 2 * ld, hipMemcpyDeviceToDevice, ctx->stream));
    MLN_TRY(triinv_solve_left_T(ctx, f->tri, w, 1, 1));
    MLN_TRY(triinv_solve_left_T(ctx, f->tri, w + ld, 1, 1));
    a.z = w;
  }
  a.ell = f->dim_ell; a.k = f->dim_k; a.mu_dim = f->mu_dim; a.mu_dens = f->mu_dens;
  a.part = f->dim_part; a.part_loss = f->part_loss; a.n_wg = f->n_wg;
  const bool hess = hess_diag != nullptr;
  if (f->n > 0) {
    MLN_TRY(launch_dim_objective(ctx, a, false));
    if (hess) MLN_TRY(launch_dim_objective(ctx, a, true));   // a second pass: four m-vectors per thread would spill
  }
  // fixed-order reduction of the partials: the four m-vectors as two "columns" blocks of 2 ld (gradients, Hessians)
  ObjArgs r{};
  r.n = f->n; r.m = 2 * ld; r.m_pad = 4 * ld; r.n_wg = f->n > 0 ? f->n_wg : 0;
  r.part_grad = f->dim_part; r.part_hess = hess ? f->dim_part + 2 * ld : nullptr; r.part_loss = f->part_loss;
  const int64_t nout = 1 + 2 * ld + (hess ? 2 * ld : 0);
  MLN_TRY(launch_reduce_obj(ctx, r, f->dim_out));
  MLN_TRY(dev_allreduce(ctx, f->dim_out, nout));
  if (f->kspace) {   // L^T v = Lp^-1 (K^T v), both gradient rows
    MLN_TRY(triinv_solve_left(ctx, f->tri, f->dim_out + 1, 1, 1));
    MLN_TRY(triinv_solve_left(ctx, f->tri, f->dim_out + 1 + ld, 1, 1));
  }
  std::vector<double> out((size_t)nout);
  MLN_HIP(ctx, hipMemcpyAsync(out.data(), f->dim_out, sizeof(double) * nout, hipMemcpyDeviceToHost, ctx->stream));
  MLN_HIP(ctx, hipStreamSynchronize(ctx->stream));
  // prior (inference.py:45-46) with the reference's k = initial_value.shape[0] = 2 latent functions:
  // 1/2 |z|^2 + (2/2) log 2 pi ; d/dz = z ; d2/dz2 = 1
  double zz = 0.0;
  for (int64_t j = 0; j < 2 * m; ++j) zz += zh[j] * zh[j];
  const double lv = out[0] + 0.5 * zz + std::log(2.0 * M_PI);
  *loss = std::isfinite(lv) ? lv : HUGE_VAL;   // a non-finite trial point reads as +inf: the line search backs off
  std::vector<double> tmp;
  double* gh = grad;
  if (is_device_ptr(grad)) { tmp.resize(2 * m); gh = tmp.data(); }
  for (int64_t j = 0; j < m; ++j) {
    gh[j] = out[1 + j] + zh[j];
    gh[m + j] = out[1 + ld + j] + zh[m + j];
  }
  if (gh != grad) MLN_HIP(ctx, hipMemcpy(grad, gh, sizeof(double) * 2 * m, hipMemcpyHostToDevice));
  if (hess) {
    std::vector<double> th;
    double* hh = hess_diag;
    if (is_device_ptr(hess_diag)) { th.resize(2 * m); hh = th.data(); }
    for (int64_t j = 0; j < m; ++j) {
      hh[j] = out[1 + 2 * ld + j] + 1.0;
      hh[m + j] = out[1 + 3 * ld + j] + 1.0;
    }
    if (hh != hess_diag) MLN_HIP(ctx, hipMemcpy(hess_diag, hh, sizeof(double) * 2 * m, hipMemcpyHostToDevice));
  }
  return MLN_OK;
}
