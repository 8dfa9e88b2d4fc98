// fp16-split row minimum for cells with 65 to 256 features (rowmin_wide.hip): pre-filter of the exact 1-NN search and
// assignment step of k-means where rowmin_f16.hip (one 64-column chunk) stops.
#pragma once
#include "mln_core.h"

constexpr int ROWMIN_WIDE_MAX_D = 256;
inline int rowmin_wide_chunks(int d) { return (d + 63) / 64; }            // 64-column chunks of a split row (2 .. 4)
inline size_t rowmin_wide_prep_doubles(int d) { return (size_t)d + 2; }   // centre [0, d), scale [d], max centred |.|^2 [d + 1]
size_t rowmin_wide_split_bytes(int64_t rows, int d);                      // device bytes of the split copy of `rows` rows

// Centre (mean of up to 4096 evenly spaced rows of y, fixed order) and power-of-two scale that puts the largest centred squared
// norm of y (and of x, if given and another set) into [2^12, 2^14).  prep: device, rowmin_wide_prep_doubles(d).
int rowmin_wide_prepare(mln_ctx* ctx, const double* y, int64_t m, const double* x, int64_t n, int d, double* prep);
// x (n x d doubles) -> split rows: per 64-column chunk hi[0..63] | lo[0..63] halves of (x - centre) * scale, zero padded.
// role 1 (query rows): the coordinates times -2; role 2 (candidate rows): as they are.  xx / xxf (either may be null): the
// squared norms of the centred, scaled rows in fp64 / rounded to fp32.
int launch_split_wide(mln_ctx* ctx, const double* x, int64_t n, int d, void* split, double* xx, float* xxf, int role,
                      const double* prep);
// per query row i: m1 = min_j (yyf_j - 2 x_i.y_j), arg = its j (the exact column), m2 = the second smallest (null: not
// tracked); exclude_self: the pair (i, i + self_offset) does not count
int launch_rowmin_wide(mln_ctx* ctx, const void* xs, int64_t n, const void* ys, int64_t m, int d, const float* yyf,
                       int64_t self_offset, int exclude_self, float* m1, float* m2, int* arg);
// E[i] = rowmin_value_bound_wide(sqrt(xx[i]), sqrt(ymax[0]), chunks(d)): what the certification allows row i
int launch_rowmin_wide_bound(mln_ctx* ctx, const double* xx, int64_t n, const double* ymax, int d, double* E);
// the winner's exact fp64 value against m2 - E: out[i] = the winner's distance (coordinate-order sum), rows not certified
// are appended to flagged[atomicAdd(n_flag)]
int launch_nn_certify_wide(mln_ctx* ctx, const double* x, int64_t n, const double* y, int64_t m, int d, const double* xx,
                           const double* yy, const float* m2, const int* arg, const double* ymax, int64_t self_offset,
                           const double* prep, double* out, int* n_flag, int* flagged);
// exact nearest-neighbour distances for 65 <= d <= 256 (nn_search_wide, rowmin_f16.hip): wide sweep + fp64 certification +
// exact re-search of the rows left open; records route 4 and the open rows in ctx->nn_last
int nn_distances_wide(mln_ctx* ctx, const double* x, int64_t n, const double* y, int64_t m, int d, int64_t self_offset, double* out);

// Bound on |s~_j - s_j| for every candidate j of a row with |x'| = xn when max_j |y'_j| = yn (centred, scaled units), c chunks.
//   s_j  = |y'_j|^2 - 2 x'.y'_j in exact arithmetic;
//   s~_j = fl32(fl32(HH + CX) + fl32(|y'_j|^2)),  HH = sum a_hi b_hi,  CX = sum a_hi b_lo + a_lo b_hi  (fp32 MFMA sums),
//   a = -2 x' = a_hi + a_lo + da and y' = b_hi + b_lo + db split into halves (hi = half(v), lo = half(v - hi)).
// Per coordinate, with the half-precision unit 2^-11 and subnormal spacing 2^-24 (|a_k| <= 256, |y'_k| <= 128: no overflow):
//   |v_lo| <= 2^-11 |v| + 2^-24,   |dv| <= 2^-22 |v| + 2^-25.
// With M = |a| |y'| = 2 xn yn (Cauchy-Schwarz), K = 64 c slots and sum_k |v_k| <= sqrt(K) |v|:
//   split     the dropped a_lo.b_lo + da.y' + (a - da).db:  <= 3.001 2^-22 M + 1.01 2^-25 sqrt(K) (2 xn + yn) + K 2^-47
//             -- taken as 2^-20 M + 2^-24 sqrt(K) (2 xn + yn) + K 2^-47;
//   HH        products of two halves are exact in fp32; an MFMA adds 16 of them to its accumulator with at most 17 roundings,
//             4 c MFMAs in the chain: relative error gamma(68 c) on sum |a_hi||b_hi| <= P = 1.002 M + 2^-24 sqrt(K) (2 xn + yn);
//   CX        8 c MFMAs: gamma(136 c) on sum |a_hi||b_lo| + |a_lo||b_hi| <= Q = 2^-10 1.002 M + 2^-23 sqrt(K) (2 xn + yn);
//   epilogue  two fp32 additions: u (P + Q) and u (P + Q + yn^2);  |y'|^2 rounded to fp32: u yn^2;
//   fp64      the norms and the reference value itself are fp64 sums of <= 256 terms: 2^-40 (M + yn^2) covers them;
// u = 2^-24, gamma(n) = n u / (1 - n u) <= 1.0001 n u for n <= 544 (folded into the 1.002).  The factor 1.25 on the whole is
// slack for the model of the matrix instruction (one rounding per addition), as in rowmin_value_bound.
__host__ __device__ inline double rowmin_value_bound_wide(double xn, double yn, int c) {
  const double u = 5.9604644775390625e-08;        // 2^-24
  const double K = 64.0 * c, sK = sqrt(K);
  const double M = 2.0 * xn * yn, lin = sK * (2.0 * xn + yn);
  const double P = 1.002 * M + u * lin;
  const double Q = 9.765625e-04 * 1.002 * M + 2.0 * u * lin;
  const double split = 9.5367431640625e-07 * M + u * lin + K * 7.105427357601002e-15;      // 2^-20, 2^-24, 2^-47
  return 1.25 * (split + (68.0 * c + 2.0) * u * P + (136.0 * c + 2.0) * u * Q + 2.0 * u * yn * yn +
                 9.094947017729282e-13 * (M + yn * yn)) + 1e-300;                            // 2^-40
}
