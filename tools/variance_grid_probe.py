"""PredictorTime.uncertainty / covariance with multi_time= through the variance grid (one mln_predict_variance_grid call)
against the per-time loop of util.make_multi_time_argument of the same commit (run by hand on the GPU box).

Product Matern52 at the C4 columns of BASELINE.md (30 + time, 2 000 centres, ls_time = 1.5), 200 times -- the setting of
the table in DESIGN.md 3.3 -- with L = chol(K_uu + 1e-6 I) and W = L^-T diag(std) attached as the density estimators attach
them (the `std` route), for a 300-point trajectory and for 20 000 queries.

Host arrays in and out on both sides, so every figure is what a caller of the Python API waits for.  One warm-up of each
variant, then REPS timed repetitions (REPS_LONG for the 20 000-query rows) with the two variants alternating; median and
[min, max] of the wall clock around the synchronous calls.  Writes the table to profiles/variance_grid_probe.txt (or the path
given as the first argument)."""
import os
import sys
import time

sys.path.insert(0, ".")
import numpy as np

import bench
from mellon_amd import _lib, cov
from mellon_amd.base_predictor import PredictorTime
from mellon_amd.conditional import _attach_uncertainty

REPS, REPS_LONG = 5, 3
ctx = _lib.default_context()
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


def compare(label, grid, loop, reps):
    """Alternate the two variants; prints one table row."""
    _, a = timed(grid)
    _, b = timed(loop)
    err = np.abs(a - b).max() / np.abs(b).max()
    del a, b
    tg, tl = [], []
    for _ in range(reps):
        tg.append(timed(grid)[0])
        tl.append(timed(loop)[0])
    mg, ml = np.median(tg), np.median(tl)
    say(f"| {label} | {mg * 1e3:.1f} [{min(tg) * 1e3:.1f}, {max(tg) * 1e3:.1f}] | {ml * 1e3:.1f} [{min(tl) * 1e3:.1f}, "
        f"{max(tl) * 1e3:.1f}] | {ml / mg:.2f} | {err:.1e} |")


def loop_over_times(p, name, x, times):
    """The loop of util.make_multi_time_argument: one single-time call per value, stacked along axis 1."""
    return np.stack([getattr(p, name)(x, time=float(t)) for t in times], axis=1)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "variance_grid_probe.txt")
    info = ctx.device_info()
    say("command: python tools/variance_grid_probe.py")
    say(f"device: {info['arch']}, {info['n_cu']} CUs; {REPS} repetitions ({REPS_LONG} for 20 000 queries) after one warm-up, "
        "variants alternating; ms, median [min, max]")
    d_state, m, n_times = 30, 2000, 200
    x_all = bench.gaussian_mixture(100_000, d_state + 1, 4)
    x_all[:, -1] = np.repeat(np.arange(8.0), x_all.shape[0] // 8 + 1)[:x_all.shape[0]]
    rng = np.random.default_rng(4)
    c = np.ascontiguousarray(x_all[rng.choice(x_all.shape[0], m, replace=False)])
    ls = 0.5 * float(np.sqrt(((x_all[:2000, None, :d_state] - c[None, :50, :d_state]) ** 2).sum(-1)).mean())
    product = cov.Matern52(ls, active_dims=slice(None, -1)) * cov.Matern52(1.5, active_dims=-1)
    p = PredictorTime(product, c, rng.normal(size=m) / np.sqrt(m), -30.0, n_obs=x_all.shape[0])
    L = np.linalg.cholesky(np.asarray(product(c, c)) + 1e-6 * np.eye(m))
    _attach_uncertainty(p, L, rng.uniform(0.05, 0.5, size=m))
    assert p._grid_std() is not None
    times = np.linspace(0.0, 7.0, n_times)
    say()
    say(f"PredictorTime, multi_time = {n_times} points, product Matern52 ({d_state} + time columns, {m} centres), W = L^-T diag(std): "
        "grid against the loop")
    say("| method, queries | grid | loop over times | loop / grid | max diff / max |")
    say("|---|---|---|---|---|")
    t = np.linspace(0.0, 1.0, 300)[:, None]
    trajectory = np.ascontiguousarray((1 - t) * x_all[0, :-1] + t * x_all[1, :-1])
    many = np.ascontiguousarray(x_all[:20_000, :-1])
    for label, xq, reps in (("300 (trajectory)", trajectory, REPS), ("20 000", many, REPS_LONG)):
        for name in ("uncertainty", "covariance"):
            compare(f"{name}, {label}", lambda: getattr(p, name)(xq, multi_time=times),
                    lambda: loop_over_times(p, name, xq, times), reps)
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
