// Row-wise nearest candidate on the fp16 matrix cores for cells with 65 to 256 features: the sweep of rowmin_f16.hip (the
// pre-filter of the exact 1-NN search, parameters.py:352-433, and the assignment step of k-means, parameters.py:243-291)
// with the feature axis cut into c = ceil(d / 64) chunks of 64 columns.
//
// Same algorithm: the doubles are centred (mean of up to 4096 evenly spaced rows, summed in a fixed order), scaled by a power
// of two that puts the largest centred squared norm in [2^12, 2^14), and split into hi + lo halves; the three products
// hi.hi + hi.lo + lo.hi are accumulated in fp32 and the sweep keeps per query row the smallest and the second-smallest value
// of  s_ij = |y_j|^2 - 2 x_i.y_j  and the arg of the smallest.  The caller certifies a row against the winner's exact fp64
// value with rowmin_value_bound_wide (rowmin_wide.h, derived there).
//
// |y|^2 is ADDED IN THE EPILOGUE from an fp32 copy, not folded into three spare k slots as roles 1 / 2 of rowmin_f16.hip do:
//   * c = ceil(d / 64) <= 4 instead of ceil((d + 3) / 64) <= 5: at d = 126 .. 128, 190 .. 192 and 254 .. 256 a whole chunk (a
//     third to a fifth of the matrix work) less, and 128 instead of 160 registers for a wave's A operands;
//   * |y|^2 stays out of the 4 c-instruction accumulation chain, whose rounding term is the largest of the bound: it meets
//     two fp32 additions instead of 68 c roundings;
//   * the epilogue runs once per stage of 128 candidates after 48 c matrix instructions: two more additions per element
//     are nothing beside them (for d <= 61, one chunk, they were half of the epilogue -- hence the folding there).
//
// Kernel shape: 4 waves x 32 query rows per workgroup, ONE wave per SIMD (the A operands of a wave's rows, c x 4 k-steps x
// {hi, lo}, are 32 c registers per lane and stay there for the whole sweep; the 32 x 32 accumulators of a stage's four
// sub-tiles, hi.hi and cross apart, are another 128).  Candidates go through LDS one (stage, chunk) unit at a time -- 128
// rows x 64 k x {hi, lo} halves = 32 KB, double buffered, row pitch 272 B as in rowmin_f16.hip -- and the accumulators persist
// across the c chunks of a stage; running minimum, second minimum and arg are updated once per stage.  arg is the exact
// candidate column.
// Off for wide cells (callers: nn_search_wide in rowmin_f16.hip, KmLevel in kmeans.hip): no cluster pruning of the 1-NN
// search and no candidate-list second sweep -- rows the certification leaves open go to the exact fp64 search -- and in
// k-means no Hamerly / group bounds and no half-precision seeding.
#include <cmath>
#include <cstdlib>

#include "mln_internal.h"

#include "rowmin_f16.h"
#include "rowmin_wide.h"

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f16v __attribute__((ext_vector_type(16)));
typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int CK = 64;               // feature columns per chunk
constexpr int CHH = 2 * CK;          // halves per (row, chunk): hi[0..63] | lo[0..63]
constexpr int RT = 128;              // candidates per stage
constexpr int PITCH = 272;           // LDS bytes per candidate row of a unit (256 + 16): conflict-free 16-byte reads
constexpr int WG_ROWS = 128;         // query rows per workgroup

// prep[k] = mean over up to 4096 evenly spaced rows of column k, four partial sums per column added in a fixed order
__global__ __launch_bounds__(1024) void k_wide_centre(const double* __restrict__ y, int64_t m, int d, double* __restrict__ prep) {
  __shared__ double part[4][ROWMIN_WIDE_MAX_D];
  const int k = threadIdx.x & 255, g = threadIdx.x >> 8;
  const int64_t cnt = m < 4096 ? m : 4096;
  const int64_t stride = m / cnt;
  double s = 0.0;
  if (k < d)
    for (int64_t r = g; r < cnt; r += 4) s += y[(r * stride) * d + k];
  part[g][k] = s;
  __syncthreads();
  if (g == 0 && k < d) prep[k] = (part[0][k] + part[1][k] + part[2][k] + part[3][k]) / (double)cnt;
  if (threadIdx.x == 0) { prep[d] = 1.0; prep[d + 1] = 0.0; }
}

// cn[i] = |x_i - centre|^2: one wave per row, the lanes' partial sums added in a fixed order
__global__ __launch_bounds__(256) void k_wide_centred_norm(const double* __restrict__ x, int64_t n, int d, const double* __restrict__ prep,
                                                           double* __restrict__ cn) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  double s = 0.0;
  for (int k = lane; k < d; k += 64) { const double t = x[row * d + k] - prep[k]; s = fma(t, t, s); }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (lane == 0) cn[row] = s;
}

// one wave per row; lane k holds the columns k, k + 64, ... (one per chunk).  C chunks: the row is C * 128 halves.
__global__ __launch_bounds__(256) void k_split_wide(const double* __restrict__ x, int64_t n, int d, int C, _Float16* __restrict__ out,
                                                    double* __restrict__ xx, float* __restrict__ xxf, int role,
                                                    const double* __restrict__ prep) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  const double sc = prep[d];
  double s = 0.0;
  for (int ch = 0; ch < C; ++ch) {
    const int k = ch * CK + lane;
    const double v0 = (k < d) ? (x[row * d + k] - prep[k]) * sc : 0.0;       // (the padding slots are written: zeros)
    s = fma(v0, v0, s);
    const double v = (role == 1) ? -2.0 * v0 : v0;
    const _Float16 hi = (_Float16)v;
    const _Float16 lo = (_Float16)(v - (double)hi);
    _Float16* dst = out + row * ((int64_t)C * CHH) + ch * CHH;
    dst[lane] = hi;
    dst[CK + lane] = lo;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (lane == 0) { if (xx) xx[row] = s; if (xxf) xxf[row] = (float)s; }
}

// The sweep.  TOP2: also the second-smallest value per row (1-NN certification); else m1 and arg only (k-means labels).
// Ragged shapes: query rows past n read row n - 1 and are not written; candidate rows past m are staged as zeros and their
// |y|^2 is +inf, so that they never win; the k padding of the last chunk is zeros in both operands (k_split_wide).
template <int C, bool TOP2>
__global__ __launch_bounds__(256) void k_rowmin_wide(const _Float16* __restrict__ Xs, int64_t n,
                                                     const _Float16* __restrict__ Ys, int64_t m,
                                                     const float* __restrict__ yyf, int64_t self_offset, int exclude_self,
                                                     float* __restrict__ out_m1, float* __restrict__ out_m2,
                                                     int* __restrict__ out_arg) {
  extern __shared__ unsigned char lds[];                      // 2 x (RT x PITCH): the unit in use and the next one
  constexpr int64_t ROWH = (int64_t)C * CHH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 31, lg = lane >> 5;
  const int64_t row0w = (int64_t)blockIdx.x * WG_ROWS + wave * 32;
  // A operands: this wave's 32 rows, k = 64 ch + 16 ks + 8 lg + e
  h8 ahi[C][4], alo[C][4];
  {
    const int64_t ar = (row0w + lr < n) ? row0w + lr : n - 1;
    const _Float16* src = Xs + ar * ROWH + 8 * lg;
#pragma unroll
    for (int ch = 0; ch < C; ++ch)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        ahi[ch][ks] = *reinterpret_cast<const h8*>(src + ch * CHH + 16 * ks);
        alo[ch][ks] = *reinterpret_cast<const h8*>(src + ch * CHH + CK + 16 * ks);
      }
  }
  float m1[16], m2[16];
  int a1[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) { m1[r] = INFINITY; m2[r] = INFINITY; a1[r] = 0; }

  // staging: a unit is 128 rows x 256 B = 2048 16-byte pieces, 8 per thread
  v4i st[8];
  auto g_load = [&](int64_t col0, int ch) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int piece = tid + 256 * q, r = piece >> 4, seg = piece & 15;
      const int64_t c = col0 + r;
      st[q] = (c < m) ? *reinterpret_cast<const v4i*>(Ys + c * ROWH + ch * CHH + seg * 8) : v4i{0, 0, 0, 0};
    }
  };
  auto l_store = [&](int buf) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int piece = tid + 256 * q, r = piece >> 4, seg = piece & 15;
      *reinterpret_cast<v4i*>(lds + buf * (RT * PITCH) + r * PITCH + seg * 16) = st[q];
    }
  };
  g_load(0, 0);
  l_store(0);
  __syncthreads();
  int buf = 0;
  for (int64_t col0 = 0; col0 < m; col0 += RT) {
    // |y|^2 of this lane's four candidates of the stage (+inf past the end), requested ahead of the products
    float yc[RT / 32];
#pragma unroll
    for (int sub = 0; sub < RT / 32; ++sub) {
      const int64_t c = col0 + sub * 32 + lr;
      yc[sub] = (c < m) ? yyf[c] : INFINITY;
    }
    f16v hh[RT / 32], cx[RT / 32];
#pragma unroll
    for (int sub = 0; sub < RT / 32; ++sub)
#pragma unroll
      for (int r = 0; r < 16; ++r) { hh[sub][r] = 0.f; cx[sub][r] = 0.f; }
#pragma unroll
    for (int ch = 0; ch < C; ++ch, buf ^= 1) {
      // the unit after this one: the next chunk of the stage, or chunk 0 of the next stage
      const bool last_ch = ch + 1 == C;
      const bool more = !last_ch || col0 + RT < m;
      if (more) g_load(last_ch ? col0 + RT : col0, last_ch ? 0 : ch + 1);
      const unsigned char* base = lds + buf * (RT * PITCH);
#pragma unroll
      for (int sub = 0; sub < RT / 32; ++sub) {
        const unsigned char* brow = base + (sub * 32 + lr) * PITCH + 16 * lg;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const h8 bhi = *reinterpret_cast<const h8*>(brow + 32 * ks);
          const h8 blo = *reinterpret_cast<const h8*>(brow + 2 * CK + 32 * ks);
          hh[sub] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi[ch][ks], bhi, hh[sub], 0, 0, 0);
          cx[sub] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi[ch][ks], blo, cx[sub], 0, 0, 0);
          cx[sub] = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo[ch][ks], bhi, cx[sub], 0, 0, 0);
        }
      }
      if (more) l_store(buf ^ 1);
      __syncthreads();
    }
    // the stage's epilogue: running minimum, second minimum and arg of every (row, column lane)
#pragma unroll
    for (int sub = 0; sub < RT / 32; ++sub) {
      const int col = (int)(col0 + sub * 32 + lr);
      // the excluded pair (i, i + self_offset) can only sit in a tile that meets this wave's diagonal band
      const int64_t lo_c = col0 + sub * 32, d0 = row0w + self_offset;
      const bool diag = exclude_self && lo_c < d0 + 32 && lo_c + 32 > d0;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float s = (hh[sub][r] + cx[sub][r]) + yc[sub];
        if (diag) {
          const int64_t row = row0w + (r & 3) + 8 * (r >> 2) + 4 * lg;
          if ((int64_t)col == row + self_offset) s = INFINITY;
        }
        if (TOP2) m2[r] = fminf(m2[r], fmaxf(m1[r], s));
        a1[r] = (s < m1[r]) ? col : a1[r];
        m1[r] = fminf(m1[r], s);
      }
    }
  }
  // merge the 32 column-lanes of each row (lanes with the same lg hold the same rows)
#pragma unroll
  for (int r = 0; r < 16; ++r) {
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) {
      const float o1 = __shfl_xor(m1[r], off, 64), o2 = __shfl_xor(m2[r], off, 64);
      const int oa = __shfl_xor(a1[r], off, 64);
      if (TOP2) m2[r] = fminf(fmaxf(m1[r], o1), fminf(m2[r], o2));
      // ties go to the smaller candidate index: the result does not depend on the lane order of the merge
      const bool take = (o1 < m1[r]) || (o1 == m1[r] && oa < a1[r]);
      a1[r] = take ? oa : a1[r];
      m1[r] = fminf(m1[r], o1);
    }
    const int64_t row = row0w + (r & 3) + 8 * (r >> 2) + 4 * lg;
    if (lr == 0 && row < n) {
      out_m1[row] = m1[r];
      if (TOP2) out_m2[row] = m2[r];
      out_arg[row] = a1[r];
    }
  }
}

__global__ void k_wide_bound(const double* __restrict__ xx, int64_t n, const double* __restrict__ ymax, int C, double* __restrict__ E) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) E[i] = rowmin_value_bound_wide(sqrt(xx[i]), sqrt(ymax[0]), C);
}

// Exact fp64 value of the winner, certification against the runner-up, list of the rows that need the exact search
// (k_nn_certify of rowmin_f16.hip with the wide prep layout and bound; arg is the exact column).
//   s_j = |y_j|^2 - 2 x.y_j (exact);  |s~_j - s_j| <= E_i for every j  =>  j* != arg implies s_{j*} >= m2~ - E_i.
__global__ __launch_bounds__(256) void k_nn_certify_wide(const double* __restrict__ x, int64_t n, const double* __restrict__ y, int64_t m, int d,
                                                         int C, const double* __restrict__ xx, const double* __restrict__ yy,
                                                         const float* __restrict__ m2, const int* __restrict__ arg,
                                                         const double* __restrict__ yy_max, int64_t self_offset,
                                                         const double* __restrict__ prep, double* __restrict__ out,
                                                         int* __restrict__ n_flag, int* __restrict__ flagged) {
  // eight lanes per row, every eighth coordinate each, partial sums added in a fixed order
  const int sub = threadIdx.x & 7;
  const int64_t i = (int64_t)blockIdx.x * 32 + (threadIdx.x >> 3);
  if (i >= n) return;                                  // (whole groups of eight leave together)
  const double sc = prep[d];
  const int64_t j = (int64_t)arg[i];
  const bool valid = j >= 0 && j < m && j != i + self_offset;
  double s = INFINITY;
  if (valid) {
    double dot = 0.0;
    for (int k = sub; k < d; k += 8) dot = fma((x[i * d + k] - prep[k]) * sc, (y[j * d + k] - prep[k]) * sc, dot);
    dot += __shfl_xor(dot, 1, 64);
    dot += __shfl_xor(dot, 2, 64);
    dot += __shfl_xor(dot, 4, 64);
    s = yy[j] - 2.0 * dot;
  }
  const double E = rowmin_value_bound_wide(sqrt(xx[i]), sqrt(yy_max[0]), C);
  const bool certified = ((double)m2[i] - E) > s;
  // reported: the winner's distance from its coordinates in order (sum (x_k - y_k)^2): exact 0 for a duplicated cell, and the
  // sum the exact search reports -- a row's value does not depend on which of them resolved it
  if (sub != 0) return;
  double dd = INFINITY;
  if (valid) {
    dd = 0.0;
    for (int k = 0; k < d; ++k) {
      const double t = x[i * d + k] - y[j * d + k];
      dd = fma(t, t, dd);
    }
  }
  out[i] = sqrt(dd);
  if (!certified) flagged[atomicAdd(n_flag, 1)] = (int)i;
}

}  // namespace

size_t rowmin_wide_split_bytes(int64_t rows, int d) { return sizeof(_Float16) * (size_t)rows * (size_t)(rowmin_wide_chunks(d) * CHH); }

static bool wide_d_ok(mln_ctx* ctx, int d) {
  if (d > CK && d <= ROWMIN_WIDE_MAX_D) return true;
  mln_set_error(ctx, "rowmin (wide): needs 65 <= d <= 256");
  return false;
}

int rowmin_wide_prepare(mln_ctx* ctx, const double* y, int64_t m, const double* x, int64_t n, int d, double* prep) {
  if (m <= 0) return MLN_OK;
  if (!wide_d_ok(ctx, d)) return MLN_ERR_UNSUPPORTED;
  const bool two = x && n > 0 && x != y;
  StreamBuf<double> cn, mx;                      // used on ctx->stream only, drained below
  MLN_TRY(cn.alloc(ctx, (size_t)(two && n > m ? n : m), "rowmin (wide): centred norms"));
  MLN_TRY(mx.alloc(ctx, 2, "rowmin (wide): maxima"));
  hipLaunchKernelGGL(k_wide_centre, dim3(1), dim3(1024), 0, ctx->stream, y, m, d, prep);
  hipLaunchKernelGGL(k_wide_centred_norm, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, ctx->stream, y, m, d, prep, cn.get());
  int rc = launch_max_norm(ctx, cn, m, mx);
  if (rc == MLN_OK && two) {
    hipLaunchKernelGGL(k_wide_centred_norm, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, ctx->stream, x, n, d, prep, cn.get());
    rc = launch_max_norm(ctx, cn, n, mx + 1);
  }
  double h[2] = {0.0, 0.0};
  if (rc == MLN_OK && hipMemcpyAsync(h, mx, sizeof(double) * (two ? 2 : 1), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = MLN_ERR_HIP;
  if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == MLN_OK) rc = MLN_ERR_HIP;
  if (rc != MLN_OK) return rc == MLN_ERR_HIP ? mln_hip_fail(ctx, hipGetLastError(), "rowmin (wide) prepare", __FILE__, __LINE__) : rc;
  // (NaN compares false: a non-finite maximum of either set leaves the scale at 1)
  const double big = (std::isfinite(h[0]) && std::isfinite(h[1])) ? (h[0] > h[1] ? h[0] : h[1]) : INFINITY;
  double tail[2] = {1.0, big};
  if (std::isfinite(big) && big > 0.0) {
    int e = 0;
    (void)std::frexp(big, &e);                                   // big = f * 2^e, f in [0.5, 1)
    const int q = 14 - e;
    tail[0] = std::ldexp(1.0, q >= 0 ? q / 2 : -((1 - q) / 2));   // floor(q / 2): big * scale^2 in [2^12, 2^14)
  }
  MLN_HIP(ctx, hipMemcpyAsync(prep + d, tail, sizeof(double) * 2, hipMemcpyHostToDevice, ctx->stream));
  MLN_HIP(ctx, hipStreamSynchronize(ctx->stream));      // (tail lives on this stack frame)
  return MLN_OK;
}

int launch_split_wide(mln_ctx* ctx, const double* x, int64_t n, int d, void* split, double* xx, float* xxf, int role,
                      const double* prep) {
  if (n <= 0) return MLN_OK;
  if (!wide_d_ok(ctx, d)) return MLN_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(k_split_wide, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, ctx->stream, x, n, d, rowmin_wide_chunks(d),
                     reinterpret_cast<_Float16*>(split), xx, xxf, role, prep);
  MLN_HIP(ctx, hipGetLastError());
  return MLN_OK;
}

template <int C>
static int launch_rowmin_wide_c(mln_ctx* ctx, const _Float16* X, int64_t n, const _Float16* Y, int64_t m, const float* yyf,
                                int64_t self_offset, int exclude_self, float* m1, float* m2, int* arg) {
  const size_t lds_bytes = (size_t)2 * RT * PITCH;              // 68 KB: above the default limit of a launch
  static bool attr = false;
  if (!attr) {
    MLN_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_rowmin_wide<C, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    MLN_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_rowmin_wide<C, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    attr = true;
  }
  const dim3 grid((unsigned)((n + WG_ROWS - 1) / WG_ROWS)), block(256);
  if (m2) hipLaunchKernelGGL((k_rowmin_wide<C, true>), grid, block, lds_bytes, ctx->stream, X, n, Y, m, yyf, self_offset, exclude_self, m1, m2, arg);
  else hipLaunchKernelGGL((k_rowmin_wide<C, false>), grid, block, lds_bytes, ctx->stream, X, n, Y, m, yyf, self_offset, exclude_self, m1, nullptr, arg);
  MLN_HIP(ctx, hipGetLastError());
  return MLN_OK;
}

int launch_rowmin_wide(mln_ctx* ctx, const void* xs, int64_t n, const void* ys, int64_t m, int d, const float* yyf,
                       int64_t self_offset, int exclude_self, float* m1, float* m2, int* arg) {
  if (n <= 0 || m <= 0) return MLN_OK;
  if (!wide_d_ok(ctx, d)) return MLN_ERR_UNSUPPORTED;
  if (m > 2147483647LL || (n + WG_ROWS - 1) / WG_ROWS > 2147483647LL) { mln_set_error(ctx, "rowmin (wide): too many rows"); return MLN_ERR_UNSUPPORTED; }
  const _Float16* X = reinterpret_cast<const _Float16*>(xs);
  const _Float16* Y = reinterpret_cast<const _Float16*>(ys);
  switch (rowmin_wide_chunks(d)) {
    case 2: return launch_rowmin_wide_c<2>(ctx, X, n, Y, m, yyf, self_offset, exclude_self, m1, m2, arg);
    case 3: return launch_rowmin_wide_c<3>(ctx, X, n, Y, m, yyf, self_offset, exclude_self, m1, m2, arg);
    default: return launch_rowmin_wide_c<4>(ctx, X, n, Y, m, yyf, self_offset, exclude_self, m1, m2, arg);
  }
}

int launch_rowmin_wide_bound(mln_ctx* ctx, const double* xx, int64_t n, const double* ymax, int d, double* E) {
  if (n <= 0) return MLN_OK;
  hipLaunchKernelGGL(k_wide_bound, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, xx, n, ymax, rowmin_wide_chunks(d), E);
  MLN_HIP(ctx, hipGetLastError());
  return MLN_OK;
}

int launch_nn_certify_wide(mln_ctx* ctx, const double* x, int64_t n, const double* y, int64_t m, int d, const double* xx,
                           const double* yy, const float* m2, const int* arg, const double* ymax, int64_t self_offset,
                           const double* prep, double* out, int* n_flag, int* flagged) {
  if (n <= 0) return MLN_OK;
  hipLaunchKernelGGL(k_nn_certify_wide, dim3((unsigned)((n + 31) / 32)), dim3(256), 0, ctx->stream, x, n, y, m, d, rowmin_wide_chunks(d),
                     xx, yy, m2, arg, ymax, self_offset, prep, out, n_flag, flagged);
  MLN_HIP(ctx, hipGetLastError());
  return MLN_OK;
}
