"""The batched objective behind optimizer="advi" on the MI355X, in one process per shape: one mln_objective call, one
mln_objective_batch call at S = 40, the same two products composed from mln_gemm (F = B W, G = B^T F on a device matrix of
the same shape; the likelihood between them is left out, so this is a lower bound of the composition), and a 100-step
run_advi on the handle.  Prints one JSON line per measurement.

    python tools/advi_probe.py --shape c3|c2 [--batch-only] [--steps 100]
    python tools/advi_probe.py --dim [--explicit] [--batch-only]

--dim measures the dimensionality objective instead (DimensionalityEstimator(optimizer="advi")): one mln_dim_objective
call, S of them, and one mln_dim_objective_batch call on the same handle at 2e5 cells x 5000 landmarks, k = 10 (synthetic
sorted distances); implicit handle unless --explicit.

Shapes: c3 = 1e6 cells x 50 dims, 5000 landmarks; c2 = 1e5 x 20, 1000; implicit handle (the estimators' default).
Landmarks are random cells and the nearest-neighbour distances synthetic: the timings do not depend on either.
Times are wall clock around synchronous library calls (median of the repetitions).  Run each invocation under its own
`timeout`; --batch-only (three batch calls, nothing else) is the body for `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"c3": (1_000_000, 50, 5000), "c2": (100_000, 20, 1000)}
FP64_MATRIX_PEAK_TFLOPS = 78.6        # MI355X spec
HBM_PEAK_GBS = 8000.0


def emit(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn, reps):
    ts = []
    out = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


class _BatchLoss:
    def __init__(self, fit):
        self.fit = fit

    def value_and_grad_batch(self, Z):
        return self.fit.objective_batch(Z)


DIM_SHAPE = (200_000, 20, 5000, 10)      # cells, dims, landmarks, neighbours
DIM_CHUNK = 32                           # samples per chunk of mln_dim_objective_batch


def dim_main(args):
    import bench
    from mellon_amd import _lib, cov
    n, d, m, k = DIM_SHAPE
    S = args.samples
    ctx = _lib.default_context()
    x = bench.gaussian_mixture(n, d, 3)
    rng = np.random.default_rng(0)
    xu = np.ascontiguousarray(x[rng.choice(n, size=m, replace=False)])
    ell = np.log(np.sort(np.abs(rng.standard_normal((n, k))) + 0.05, axis=-1)) + np.log(np.pi) / 2
    fit = ctx.fit_prepare(cov.Matern52(float(np.sqrt(d))).lower(d), x, xu, 1e-6, implicit=not args.explicit)
    fit.set_dim_likelihood(ell, 0.3, 1.1)
    Z = 0.05 * rng.standard_normal((S, 2, m))
    fit.dim_objective_batch(Z[:2])                # module load, Lp factorisation
    fit.dim_objective_batch(Z)
    fit.dim_objective(Z[0])
    if args.batch_only:
        for _ in range(3):
            fit.dim_objective_batch(Z)
        return
    chunks = (S + DIM_CHUNK - 1) // DIM_CHUNK
    common = dict(shape="dim", handle="explicit" if args.explicit else "implicit", n=n, m=m, k=k, S=S)
    # the two versions alternate, so that a change of the machine's load between them shows in the spread
    t_single, t_batch = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        singles = [fit.dim_objective(z) for z in Z]
        t1 = time.perf_counter()
        loss, grad = fit.dim_objective_batch(Z)
        t2 = time.perf_counter()
        t_single.append(t1 - t0)
        t_batch.append(t2 - t1)
    e_loss = max(abs(loss[s] - singles[s][0]) / abs(singles[s][0]) for s in range(S))
    e_grad = max(np.abs(grad[s] - singles[s][1]).max() / np.abs(singles[s][1]).max() for s in range(S))
    ts, tb = float(np.median(t_single)), float(np.median(t_batch))
    emit(what="dim_objective_x_S", seconds=ts, min=min(t_single), max=max(t_single), **common)
    emit(what="dim_objective_batch", seconds=tb, min=min(t_batch), max=max(t_batch), ratio_to_S_single_passes=tb / ts,
         speedup=ts / tb, speedup_from_traffic_alone=S / (2.0 * chunks), buffer_reads=2 * chunks,
         buffer_gb_per_s=2 * chunks * 8.0 * n * m / tb / 1e9, max_rel_loss_diff=e_loss, max_rel_grad_diff=e_grad, **common)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", action="store_true")
    ap.add_argument("--explicit", action="store_true")
    ap.add_argument("--shape", choices=sorted(SHAPES), default="c3")
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--batch-only", action="store_true")
    args = ap.parse_args()
    if args.dim:
        return dim_main(args)
    import bench
    from mellon_amd import _lib, cov, inference
    n, d, m = SHAPES[args.shape]
    S = args.samples
    ctx = _lib.default_context()
    x = bench.gaussian_mixture(n, d, 3)
    rng = np.random.default_rng(0)
    xu = np.ascontiguousarray(x[rng.choice(n, size=m, replace=False)])
    r = rng.uniform(0.5, 1.5, size=n)
    const = d * np.log(np.pi) / 2 - float(__import__("scipy.special").special.gammaln(d / 2 + 1))
    V = d * np.log(r) + const
    Vdr = np.log(d) + (d - 1) * np.log(r) + const
    mu = -float(np.mean(V))
    fit = ctx.fit_prepare(cov.Matern52(float(np.sqrt(d))).lower(d), x, xu, 1e-6, implicit=True)
    fit.set_likelihood(V, Vdr, mu)
    Z = 0.05 * rng.standard_normal((S, m))
    fit.objective_batch(Z[:2])                    # module load, Lp factorisation
    fit.objective(Z[0])
    SP = 16 * ((S + 15) // 16)
    common = dict(shape=args.shape, n=n, m=m, S=S)
    if args.batch_only:
        for _ in range(3):
            fit.objective_batch(Z)
        return
    t1, _ = timed(lambda: fit.objective(Z[0]), 5)
    emit(what="objective", seconds=t1, **common)
    t40, _ = timed(lambda: [fit.objective(z) for z in Z], 3)
    emit(what="objective_x_S", seconds=t40, **common)
    tb, _ = timed(lambda: fit.objective_batch(Z), 5)
    flop = 2 * 2.0 * n * m * SP
    emit(what="objective_batch", seconds=tb, ratio_to_S_single_passes=tb / t40, bar=1.0 / 3.0,
         tflops=flop / tb / 1e12, fraction_of_fp64_matrix_peak=flop / tb / 1e12 / FP64_MATRIX_PEAK_TFLOPS,
         buffer_gb_per_s=2 * 8.0 * n * m / tb / 1e9, fraction_of_hbm_peak=2 * 8.0 * n * m / tb / 1e9 / HBM_PEAK_GBS, **common)
    # yardstick: the two products alone through mln_gemm, on a device matrix of the buffer's shape
    B = ctx.gemm(rng.uniform(0.0, 1.0, size=(n, 1)), rng.uniform(0.0, 1.0, size=(1, m)))
    W = ctx.to_device(np.ascontiguousarray(Z.T))
    F = ctx.empty((n, S))
    G = ctx.empty((m, S))

    def pair():
        ctx.gemm(B, W, out=F)
        ctx.gemm(B, F, ta=True, out=G)
        ctx.synchronize()

    pair()
    tg, _ = timed(pair, 3)
    emit(what="mln_gemm_pair", seconds=tg, batch_over_gemm_pair=tb / tg, **common)
    for a in (B, W, F, G):
        a.free()
    t0 = time.perf_counter()
    res = inference.run_advi(_BatchLoss(fit), np.zeros(m), n_iter=args.steps, nsamples=S)
    tf = time.perf_counter() - t0
    emit(what="run_advi", steps=args.steps, seconds=tf, seconds_per_step=tf / args.steps,
         loss_first=float(res.losses[0]), loss_last=float(res.losses[-1]), **common)


if __name__ == "__main__":
    main()
