// What the batched objectives share (objective_batch.hip: mln_objective_batch; dim_objective_batch.hip:
// mln_dim_objective_batch): the tile constants of the two skinny fp64 MFMA products, the backward product
// G = B^T C with its fixed-order partial sums, and the per-sample sum of the forward kernels' likelihood partials.
// Each including file gets its own copy of the kernels (anonymous namespace); the forward kernels differ and stay in their files.
#pragma once
#include "api_internal.h"

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

constexpr int BT = 256;           // buffer rows (forward) / buffer columns (backward) of a workgroup's tile
constexpr int BK = 16;            // depth of one staged tile
constexpr int A_LD = BK + 4;      // forward: buffer tile row-major [row][k]; 20 doubles: the 16 rows x 4 k of an operand read hit distinct bank pairs
constexpr int B_LD = BT + 16;     // backward: buffer tile k-major [k][column] (as in dgemm.hip: the four k-groups on disjoint banks)

// leading dimension of the staged skinny operand ([k][SP]): an odd multiple of 16 doubles
template <int NT> struct SkinnyLd { static constexpr int v = (NT % 2) ? 16 * NT : 16 * NT + 16; };

template <int NT>
__global__ __launch_bounds__(256, 2) void k_batch_backward(const double* __restrict__ B, int64_t ldb, int64_t n,
                                                          int64_t rows_per_range, const double* __restrict__ A1,
                                                          double* __restrict__ part) {
  constexpr int SP = 16 * NT, WLD = SkinnyLd<NT>::v;
  __shared__ __attribute__((aligned(16))) double Bs[BK][B_LD];
  __shared__ double Cs[BK][WLD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lk = lane >> 4, li = lane & 15;
  const int64_t c0 = (int64_t)blockIdx.x * BT;
  const int64_t rbeg = (int64_t)blockIdx.y * rows_per_range;               // a multiple of 16
  const int64_t rend = (rbeg + rows_per_range < n) ? (rbeg + rows_per_range) : n;

  v4d acc[4][NT];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};

  d2 rb[8];
  double rc[NT];
  // buffer tile: 16 cells x 256 columns, 128 consecutive lanes read 2 KB of one row; coefficient tile: 16 cells x SP, contiguous
  auto load_tiles = [&](int64_t k0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int idx = t + 256 * q;
      const int64_t gr = k0 + (idx >> 7), gc = c0 + 2 * (idx & 127);
      rb[q] = (gr < rend && gc < ldb) ? __builtin_nontemporal_load(reinterpret_cast<const d2*>(B + gr * ldb + gc)) : (d2){0.0, 0.0};
    }
#pragma unroll
    for (int q = 0; q < NT; ++q) {
      const int idx = t + 256 * q;
      rc[q] = (k0 + idx / SP < rend) ? A1[k0 * SP + idx] : 0.0;
    }
  };
  if (rbeg < rend) load_tiles(rbeg);
  for (int64_t k0 = rbeg; k0 < rend; k0 += BK) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int idx = t + 256 * q;
      *reinterpret_cast<d2*>(&Bs[idx >> 7][2 * (idx & 127)]) = rb[q];
    }
#pragma unroll
    for (int q = 0; q < NT; ++q) {
      const int idx = t + 256 * q;
      Cs[idx / SP][idx % SP] = rc[q];
    }
    __syncthreads();
    if (k0 + BK < rend) load_tiles(k0 + BK);
#pragma unroll
    for (int kk = 0; kk < BK; kk += 4) {
      double a[4], b[NT];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = Bs[kk + lk][wave * 64 + i * 16 + li];
#pragma unroll
      for (int j = 0; j < NT; ++j) b[j] = Cs[kk + lk][j * 16 + li];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }
  double* out = part + (int64_t)blockIdx.y * ldb * SP;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t c = c0 + wave * 64 + i * 16 + lk + 4 * r;
      if (c < ldb) {
#pragma unroll
        for (int j = 0; j < NT; ++j) out[c * SP + j * 16 + li] = acc[i][j][r];
      }
    }
}

// out[i] = sum_p parts[p][i], p ascending
__global__ __launch_bounds__(256) void k_batch_sum(const double* __restrict__ parts, int n_parts, int64_t stride,
                                                   double* __restrict__ out, int64_t count) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  double s = 0.0;
  for (int p = 0; p < n_parts; ++p) s += parts[(int64_t)p * stride + i];
  out[i] = s;
}

// likelihood sum of sample blockIdx.x over the row tiles: strided per-thread sums, then a fixed tree
__global__ __launch_bounds__(256) void k_batch_loss_sum(const double* __restrict__ part_loss, int64_t n_tiles, int SP,
                                                        double* __restrict__ out) {
  __shared__ double red[256];
  const int s = blockIdx.x, t = threadIdx.x;
  double l = 0.0;
  for (int64_t w = t; w < n_tiles; w += 256) l += part_loss[w * SP + s];
  red[t] = l;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (t < off) red[t] += red[t + off];
    __syncthreads();
  }
  if (t == 0) out[s] = red[0];
}

}  // namespace
