// Importance-sampled rows for the solver's second preconditioner (precond_rebuild.hip).
#pragma once
#include "mln_core.h"

struct RebuildSelection {
  int64_t rows = 0;        // selected rows of THIS rank
  DevBuf<int64_t> idx;     // their local indices, ascending (device)
  DevBuf<double> scale;    // sqrt(w_i / w_max) per selected row (device) -- or, asked for, 1 / p_i
  double w_max = 1.0;      // global; the Gram of the scaled rows times w_max estimates sum_i a_i L_i L_i^T
  double c = 0.0;          // p_i = min(1, c a_i)
  double sum_a = 0.0;      // global sum of the weights
  void reset() { idx.reset(); scale.reset(); rows = 0; }   // (the caller has drained the stream)
};

// f_dev, V_dev: n rows of this rank (f = L z + mu at the solver's accepted point); row0: global index of its first cell.
// Collective: every rank calls it (all-reduces of the weight sums).
int rebuild_select_rows(mln_ctx* ctx, const double* f_dev, const double* V_dev, int64_t n, int64_t row0,
                        double target_rows_global, uint64_t seed, RebuildSelection* out, double cap = 1e300,
                        bool inverse_prob = false);
// (cap: weights are e^{min(f + V, cap)} -- the second derivative of the solver's capped likelihood term)
// (inverse_prob: `scale` holds 1 / p_i = max(1, 1 / (c a_i)) instead -- the weights of an unbiased sum over the selected
//  rows, the importance tail of the MAP solve.  Same seed, larger target: a superset of the smaller draw.)
int launch_gather_scale_rows(mln_ctx* ctx, const double* A, int64_t ld, const int64_t* idx, const double* scale,
                             int64_t rows, double* R);
