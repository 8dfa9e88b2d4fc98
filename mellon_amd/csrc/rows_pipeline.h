// The persistent-row tile pipeline of the covariance kernels, written once: the kernel-matrix pass of the fit
// (cov_rows_impl.h) and the fused predictive mean (predict_rows_impl.h), each for one stationary leaf and for the
// time-sensitive product of two, are this pipeline with their own per-element epilogue.
//
// A workgroup of 8 waves owns 128 rows; every wave keeps the MFMA A operands of its 16 rows in registers and walks all
// centre tiles (staged through LDS).  In one loop body the wave issues the 4 x KSTEPS MFMAs of tile t+1 into one
// accumulator set while the epilogue of tile t runs on the other set -- independent instruction streams in one basic
// block, interleaved with sched_group_barrier, so neither the matrix pipe nor the VALU waits for the other.
//
// What makes it fast is a set of contracts (counters: profiles/r02_pmc_sq.txt, profiles/r03_pmc_sq.txt):
//   * Padded copies.  `y`, `yy` and `w` are COPIES of the centres, their squared norms and their weights followed by
//     3 TN zero rows (cov_kernels.hip: ROWS_PAD; the kernel-matrix pass takes these kernels only while ldo <= m + 64).
//     The staging therefore needs neither address clamps nor value masks: a staged load is
//     `global_load v, v_off32, s[tile base]` with a byte offset that never changes, its LDS destination a constant per
//     thread; a thread without an element loads offset 0 and stores to a sink slot of its own behind the tile.
//   * The barrier of the tile loop waits for LDS traffic only (`s_waitcnt lgkmcnt(0)` + `s_barrier`).  __syncthreads()
//     is a full fence, i.e. vmcnt(0): every wave would sit out the acknowledgement of the stores its epilogue has just
//     issued, once per tile.
//   * Centre tile t+2 is REQUESTED at the top of the body (global loads into registers) and written to LDS at the bottom.
//     Nothing in between may consume a load, so the wait before the LDS writes is vmcnt(#stores issued since), not
//     vmcnt(0).
//   * FAST tiles (branch-free epilogue) and the others run in SEPARATE loops: a branch between the two inside one loop
//     makes the compiler assume the slow path's unknown store count at the join, and the wait above drains everything.
//   * The tile loop is unrolled by two, so that the two accumulator sets swap roles instead of being copied (16 v_mov_b64
//     per tile) and every LDS address of the operand tiles is an immediate.
#pragma once
#include <type_traits>
#include "cov_rows.h"
#include "cov_epilogue.h"

namespace rowspipe {
using covrows::NNS;
using covrows::TN;

__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// A lane's place in the 8-wave x 16-row layout: after an MFMA, accumulator element [tt][r] belongs to row
// row0 + lk + 4 r and to column 16 tt + li of the tile.
struct Lane {
  int tid, li, lk, wave;
  int64_t row0;       // first row of the wave
  __device__ __forceinline__ int64_t row(int r) const { return row0 + lk + 4 * r; }
};
__device__ __forceinline__ Lane lane() {
  const int tid = threadIdx.x, l = tid & 63, wave = tid >> 6;
  return Lane{tid, l & 15, l >> 4, wave, (int64_t)blockIdx.x * 128 + wave * 16};
}

// Per-centre side values, in the order of their LDS buffers: the scaled squared norm always; with TIME the scaled time
// stamp (the LAST column of x and y, which is then no MFMA operand); with WEIGHT the weight (0 behind the last centre:
// that masks the pad columns).
constexpr int SIDE_NORM = 0, SIDE_TIME = 1;
constexpr int side_weight(bool TIME) { return TIME ? 2 : 1; }
constexpr int SIDE_STRIDE = 3 * 512;   // three buffers each: the epilogue of tile t reads them one step after tile t+2 is staged
struct SideTile {                      // the side values of one tile as the lane reads them: value k of column 16 tt + li
  const double* p;
  __device__ __forceinline__ double operator()(int k, int tt) const { return p[k * SIDE_STRIDE + 16 * tt]; }
};

// Walks all `ntiles` centre tiles.  `epi(cur, side, col0, fast_tag)` is the epilogue of one tile: `cur` its dot products,
// `side` its side values, `col0` its first column; the first `n_fast` tiles (rounded down to even) are announced with
// std::true_type and must then be branch-free.  With SLOW_TAIL the remaining tiles follow with std::false_type, one
// step at a time and with the staging clamped to the last tile; without it n_fast == ntiles, and the tiles requested
// past the end lie within the padding: (ntiles + 2) TN < m + 3 TN.
// c2 and c1 scale the squared norms and the time stamps.  EPI_VALU is the VALU instruction count of one FAST epilogue
// per lane, spread evenly between the MFMAs; 0 leaves the order to the scheduler.
template <int KSTEPS, bool TIME, bool WEIGHT, bool SLOW_TAIL, int EPI_VALU, class Epilogue>
__device__ __forceinline__ void rows_pipeline(const double* __restrict__ x, int64_t n, const double* __restrict__ y, int d,
                                              const double* __restrict__ yy, const double* __restrict__ w, double c2,
                                              double c1, int64_t ntiles, int64_t n_fast, Epilogue&& epi) {
  constexpr int YB = TN * NNS + 512;   // one operand buffer: the tile, then a slot per thread for stores without an element
  constexpr int NSIDE = 1 + (TIME ? 1 : 0) + (WEIGHT ? 1 : 0);
  __shared__ double ys[2][YB];         // tile t+1 is consumed while tile t+2 lands in the buffer tile t left
  __shared__ double side[NSIDE][3][512];   // [..][..][tid < TN] used, the rest absorbs the other threads' stores
  constexpr int NST = (TN * (4 * KSTEPS + (TIME ? 1 : 0)) + 511) / 512;   // staging registers per thread: TN x d values
  const Lane L = lane();
  const int tid = L.tid, li = L.li, lk = L.lk;
  const int ds = TIME ? d - 1 : d;     // operand columns
  double a[KSTEPS];
  {
    const int64_t ar = (L.row0 + li < n) ? L.row0 + li : n - 1;
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
      const int k = 4 * ks + lk;
      a[ks] = (k < ds) ? x[ar * d + k] : 0.0;
    }
  }
  for (int e = tid; e < 2 * YB; e += 512) (&ys[0][0])[e] = 0.0;
  __syncthreads();
  const int cnt = TN * d;
  // element e of a tile: centre e / d, column e % d; its global byte offset within a tile and its LDS slot never change.
  // A time stamp is fetched once more by the thread that owns the centre's norm (the tile copy of that column goes to
  // the sink) and takes the side values' route.
  unsigned goffb[NST];
  double* dst[NST];
#pragma unroll
  for (int i = 0; i < NST; ++i) {
    const int e = tid + 512 * i;
    const int r = e / d, k = e - r * d;
    goffb[i] = (e < cnt) ? (unsigned)e * 8u : 0u;
    dst[i] = (e < cnt && (!TIME || k < ds)) ? &ys[0][r * NNS + k] : &ys[0][TN * NNS + tid];
  }
  const unsigned nb = (unsigned)(tid & (TN - 1)) * 8u;
  const unsigned tb = ((unsigned)(tid & (TN - 1)) * (unsigned)d + (unsigned)ds) * 8u;
  double sreg[NST], snorm = 0.0, stime = 0.0, sw = 0.0;
  auto stage_load = [&](int64_t tile) {          // raw values only: nothing here may CONSUME a load
    const char* ytile = (const char*)(y + tile * TN * d);
#pragma unroll
    for (int i = 0; i < NST; ++i) sreg[i] = *(const double*)(ytile + goffb[i]);
    if (TIME) stime = *(const double*)(ytile + tb);
    snorm = *(const double*)((const char*)(yy + tile * TN) + nb);
    if (WEIGHT) sw = *(const double*)((const char*)(w + tile * TN) + nb);
  };
  auto stage_store = [&](int par, int nbuf) {    // after the epilogue's stores have been issued
#pragma unroll
    for (int i = 0; i < NST; ++i) dst[i][par * YB] = sreg[i];
    side[SIDE_NORM][nbuf][tid] = c2 * snorm;
    if (WEIGHT) side[side_weight(TIME)][nbuf][tid] = sw;
    if (TIME) side[SIDE_TIME][nbuf][tid] = c1 * stime;
  };
  auto mma = [&](int buf, v4d_t (&acc)[4]) {
    const double* yb = &ys[buf][li * NNS + lk];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = v4d_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks)   // 4 KSTEPS >= ds; k columns past ds are zero in both operands
#pragma unroll
      for (int t = 0; t < 4; ++t)
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], yb[16 * t * NNS + 4 * ks], acc[t], 0, 0, 0);
  };
  stage_load(0); stage_store(0, 0);
  if (!SLOW_TAIL || ntiles > 1) { stage_load(1); stage_store(1, 1); }   // (without a clamp tile 1 exists at least as padding)
  __syncthreads();
  v4d_t accA[4], accB[4];
  mma(0, accA);
  lds_barrier();
  // One tile step: the epilogue of tile t (accumulators `cur`) while the MFMAs of tile t+1 fill `nxt`.  In a FAST step
  // the MFMAs, the epilogue and its stores form one basic block.  PAR = t & 1 and is a compile-time constant in the
  // unrolled loop; ncur = t % 3.
  auto step = [&](int64_t t, v4d_t (&cur)[4], v4d_t (&nxt)[4], int par, int ncur, auto fast_tag) {
    constexpr bool FAST = decltype(fast_tag)::value;
    const int64_t t2 = FAST ? (t + 2) : ((t + 2 < ntiles) ? (t + 2) : (ntiles - 1));   // (a clamped re-load near the end)
    stage_load(t2);                                   // requested now, written to LDS after the epilogue
    mma(par ^ 1, nxt);                                // tile t + 1 (the last one is a dummy on stale data or padding)
    epi(cur, SideTile{&side[0][ncur][li]}, t * TN, fast_tag);
    if (FAST && EPI_VALU > 0) {
#pragma unroll
      for (int i = 0; i < 4 * KSTEPS; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                         // one MFMA
        __builtin_amdgcn_sched_group_barrier(0x002, EPI_VALU / (4 * KSTEPS), 0);   // its share of the epilogue VALU
      }
    }
    stage_store(par, (ncur == 0) ? 2 : ncur - 1);     // tile t + 2: the ys buffer of tile t (its MFMAs finished last step), side buffer (t + 2) % 3
    lds_barrier();
  };
  int64_t t = 0;
  int nc = 0;
  for (; t + 2 <= n_fast; t += 2) {
    step(t, accA, accB, 0, nc, std::true_type{});
    nc = (nc == 2) ? 0 : nc + 1;
    step(t + 1, accB, accA, 1, nc, std::true_type{});
    nc = (nc == 2) ? 0 : nc + 1;
  }
  if (!SLOW_TAIL) {
    if (t < ntiles) step(t, accA, accB, 0, nc, std::true_type{});   // odd tile count (t is even here)
    return;
  }
  for (; t < ntiles; ++t) {
    step(t, accA, accB, (int)(t & 1), nc, std::false_type{});
    nc = (nc == 2) ? 0 : nc + 1;
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) accA[tt] = accB[tt];
  }
}

}  // namespace rowspipe
