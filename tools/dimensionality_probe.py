"""DimensionalityEstimator kernels on the MI355X: mln_knn (K = 30), mln_local_dimensionality, one mln_dim_objective pass
next to one mln_objective pass on the same handle, the estimator end to end, and a CPU baseline of the restated
objective.  Prints one JSON line per measurement.

    python tools/dimensionality_probe.py [--n N] [--fit-n N] [--knn-budget SECONDS]

The k-NN search is timed at 2e5 cells first; the C3 size (1e6 x 50) runs only when the n^2 projection of that time stays
within --knn-budget.  Times are wall clock around synchronous library calls (median of the repetitions)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=50)
    ap.add_argument("--m", type=int, default=5000)
    ap.add_argument("--fit-n", type=int, default=200_000)
    ap.add_argument("--fit-m", type=int, default=1000)
    ap.add_argument("--knn-budget", type=float, default=60.0)
    ap.add_argument("--passes-only", action="store_true", help="only the two objective passes (for a kernel trace)")
    args = ap.parse_args()
    import bench
    import mellon_amd
    from mellon_amd import _lib, cov
    ctx = _lib.default_context()
    x = bench.gaussian_mixture(args.n, args.d, 3)

    if args.passes_only:
        return objective_passes(ctx, cov, x, args)

    # k-NN, K = 30, and the local dimension of every query
    n_small = min(200_000, args.n)
    xs = np.ascontiguousarray(x[:n_small])
    ctx.knn(xs[:1000], 30)                      # (module load)
    t, (dist, idx) = timed(lambda: ctx.knn(xs, 30), 2)
    emit(what="mln_knn", n=n_small, d=args.d, k=30, seconds=t, pair_gflop_per_s=2.0 * n_small * n_small * args.d / t / 1e9)
    t_ld, _ = timed(lambda: ctx.local_dimensionality(xs, idx), 2)
    emit(what="mln_local_dimensionality", q=n_small, d=args.d, k=30, seconds=t_ld)
    proj = t * (args.n / n_small) ** 2
    if args.n > n_small and proj <= args.knn_budget:
        t, (dist, idx) = timed(lambda: ctx.knn(x, 30), 1)
        emit(what="mln_knn", n=args.n, d=args.d, k=30, seconds=t, pair_gflop_per_s=2.0 * args.n ** 2 * args.d / t / 1e9)
        t_ld, _ = timed(lambda: ctx.local_dimensionality(x, idx), 1)
        emit(what="mln_local_dimensionality", q=args.n, d=args.d, k=30, seconds=t_ld)
    elif args.n > n_small:
        emit(what="mln_knn", n=args.n, skipped=True, projected_seconds=proj)

    objective_passes(ctx, cov, x, args)
    rng = np.random.default_rng(1)

    # the estimator end to end
    xf = np.ascontiguousarray(x[:args.fit_n])
    est = mellon_amd.DimensionalityEstimator(n_landmarks=args.fit_m)
    t0 = time.perf_counter()
    dim = est.fit_predict(xf)
    emit(what="DimensionalityEstimator.fit_predict", n=args.fit_n, d=args.d, m=args.fit_m, seconds=time.perf_counter() - t0,
         evaluations=int(est.loss_func.n_eval), median_local_dim=float(np.median(dim)))

    # CPU baseline: the restated loss + gradient (NumPy) at reduced size
    import dim_restatement as dr
    nc, mc = 20_000, 500
    L = rng.normal(size=(nc, mc)) * 0.05
    ell = np.log(np.sort(rng.uniform(0.5, 2.0, size=(nc, 10)), axis=1)) + np.log(np.pi) / 2
    zc = rng.normal(size=(2, mc)) * 1e-3
    t_cpu, _ = timed(lambda: (dr.dim_loss(zc, L, ell, 0.0, -2.0), dr.dim_grad_hess(zc, L, ell, 0.0, -2.0)), 3)
    emit(what="cpu_restatement_loss_grad_hess", n=nc, m=mc, seconds=t_cpu,
         threads=os.environ.get("OMP_NUM_THREADS", "unset"))


def objective_passes(ctx, cov, x, args):
    """One objective pass of each kind on the same implicit handle (the default route: the n x m kernel matrix is
    streamed, Lp^-T / Lp^-1 applied to the m-vectors around each pass)."""
    rng = np.random.default_rng(0)
    lm = np.ascontiguousarray(x[rng.choice(args.n, args.m, replace=False)])
    fit = ctx.fit_prepare(cov.Matern52(bench_ls(x)).lower(args.d), x, lm, 1e-6, implicit=True)
    V = np.full(args.n, -1.0)
    fit.set_likelihood(V, V, 0.0)
    fit.set_dim_likelihood(np.log(np.sort(rng.uniform(0.5, 2.0, size=(args.n, 10)), axis=1)) + np.log(np.pi) / 2, 0.0, -2.0)
    z1 = rng.normal(size=args.m) * 1e-3
    z2 = rng.normal(size=(2, args.m)) * 1e-3
    fit.objective(z1), fit.dim_objective(z2)
    t_obj, _ = timed(lambda: fit.objective(z1), 7)
    t_dim, _ = timed(lambda: fit.dim_objective(z2), 7)
    emit(what="objective_pass", n=args.n, m=args.m, mln_objective_s=t_obj, mln_dim_objective_s=t_dim, ratio=t_dim / t_obj,
         bytes_per_pass=args.n * (args.m + (-args.m) % 16) * 8)
    fit.close()


def bench_ls(x):
    from mellon_amd import _lib
    nn = _lib.default_context().nn_distances(x[:200_000])
    return float(np.exp(np.mean(np.log(nn)) + 3.0))


if __name__ == "__main__":
    main()
