// sign and log|det| of many small matrices (numpy.linalg.slogdet's conventions): what Predictor.hessian_log_determinant
// (base_predictor.py:523-539, 1162-1194) asks of the Hessians -- 2 numbers per matrix leave the device instead of k^2.
//
// One wavefront per matrix, lane i owns row i (lead <= 64).  The lead x lead block is staged into LDS with an ODD leading
// dimension ld = lead | 1: a column walk (lane i reads a[i][c], 8 bytes at dword 2 (i ld + c)) then touches the dword pairs
// 2 i mod 64 of a 32-lane half -- all 64 banks once (the 8-byte stores of the update go in groups of 16 lanes over 32 banks:
// 16 dword pairs, again every bank once); row walks (the swap, the staging) are consecutive addresses, the pivot row is a
// broadcast.  Right-looking LU with partial pivoting: the pivot of column c is max_i>=c |a_ic| by a butterfly
// reduction over (value, row), ties to the lowest row as LAPACK's idamax; sign = (-1)^swaps prod sign(u_cc), logabsdet =
// sum_c log|u_cc| in the order c = 0 .. lead-1.  A zero pivot column ends the matrix with (0, -inf).
#include <cmath>
#include "mln_internal.h"

namespace {

__global__ __launch_bounds__(64) void k_slogdet_batched(const double* __restrict__ A, int64_t count, int k, int64_t lda,
                                                        int lead, int ld, double* __restrict__ sign,
                                                        double* __restrict__ logabs, int64_t inner, int64_t out_stride,
                                                        int64_t out_off) {
  extern __shared__ double s[];
  const int lane = threadIdx.x;
  const bool row = lane < lead;
  for (int64_t idx = blockIdx.x; idx < count; idx += gridDim.x) {
    const double* __restrict__ Am = A + idx * lda;
    __syncthreads();                                  // the previous matrix is finished with before it is overwritten
    if (row)
      for (int r = 0; r < lead; ++r) s[r * ld + lane] = Am[(int64_t)r * k + lane];
    __syncthreads();
    double sg = 1.0, la = 0.0;
    for (int c = 0; c < lead; ++c) {
      double v = (row && lane >= c) ? fabs(s[lane * ld + c]) : -1.0;
      int pi = lane;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double v2 = __shfl_xor(v, off, 64);
        const int p2 = __shfl_xor(pi, off, 64);
        if (v2 > v || (v2 == v && p2 < pi)) { v = v2; pi = p2; }
      }
      if (!(v > 0.0)) { sg = 0.0; la = -INFINITY; break; }      // (the same v on every lane: uniform)
      if (pi != c) {
        if (row && lane >= c) {                       // columns left of c hold nothing that is read again
          const double t = s[c * ld + lane];
          s[c * ld + lane] = s[pi * ld + lane];
          s[pi * ld + lane] = t;
        }
        sg = -sg;
        __syncthreads();
      }
      const double piv = s[c * ld + c];
      if (piv < 0.0) sg = -sg;
      la += log(fabs(piv));
      if (row && lane > c) {
        const double l = s[lane * ld + c] / piv;
        for (int j = c + 1; j < lead; ++j) s[lane * ld + j] -= l * s[c * ld + j];
      }
      __syncthreads();
    }
    if (lane == 0) {
      const int64_t o = (idx / inner) * out_stride + out_off + idx % inner;
      sign[o] = sg;
      logabs[o] = la;
    }
  }
}

}  // namespace

// Result idx goes to sign / logabs [(idx / inner) out_stride + out_off + idx % inner]: (count, 1, 0) is idx itself; a block of
// pb outputs of n x p results is (pb, p, q0).  Asynchronous on ctx->stream; 1 <= lead <= min(k, SLOGDET_MAX_LEAD) is the caller's.
int launch_slogdet_batched(mln_ctx* ctx, const double* A, int64_t count, int k, int64_t lda, int lead, double* sign,
                           double* logabs, int64_t inner, int64_t out_stride, int64_t out_off) {
  if (count <= 0) return MLN_OK;
  if (lead < 1 || lead > k || lead > SLOGDET_MAX_LEAD) {
    mln_set_error(ctx, "slogdet_batched: the leading block must be 1 .. min(k, 64)");
    return MLN_ERR_UNSUPPORTED;
  }
  const int ld = lead | 1;
  const int64_t blocks = count < ((int64_t)1 << 22) ? count : ((int64_t)1 << 22);
  hipLaunchKernelGGL(k_slogdet_batched, dim3((unsigned)blocks), dim3(64), sizeof(double) * (size_t)lead * ld, ctx->stream, A,
                     count, k, lda, lead, ld, sign, logabs, inner, out_stride, out_off);
  MLN_HIP(ctx, hipGetLastError());
  return MLN_OK;
}
