"""One multi-output device call against its per-output loop (run by hand on the GPU box):

  * Context.predict_gradient with (m, p) weights against p single-output calls, p in {2, 8, 64}, for a single Matern52
    leaf and for the time-sensitive product kernel, 100 000 queries x 2 000 centres x 30 (+ 1) columns;
  * PredictorTime.mean / gradient / time_derivative with multi_time = 200 points through the grid path against the
    per-time loop of util.make_multi_time_argument, at the C4 shape of BASELINE.md (5e5 queries, 30 + time columns,
    2 000 centres, product Matern52, ls_time = 1.5); the time derivative on 100 000 and the gradient on 20 000 of those
    queries (the gradient's result is n x 200 x 30).

Host arrays in and out on both sides, so every figure is what a caller of the Python API waits for.  One warm-up of each
variant, then REPS timed repetitions with the two variants alternating; median and [min, max] of the wall clock around the
synchronous calls.  Writes the table to profiles/grad_multi_probe.txt (or the path given as the first argument)."""
import os
import sys
import time

sys.path.insert(0, ".")
import numpy as np

import bench
from mellon_amd import _lib, cov
from mellon_amd.base_predictor import PredictorTime

REPS = 5
ctx = _lib.default_context()
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


def compare(label, batched, loop, reps=REPS):
    """Alternate the two variants; returns nothing, prints one table row."""
    _, a = timed(batched)
    _, b = timed(loop)
    err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
    del a, b
    tb, tl = [], []
    for _ in range(reps):
        tb.append(timed(batched)[0])
        tl.append(timed(loop)[0])
    mb, ml = np.median(tb), np.median(tl)
    say(f"| {label} | {mb * 1e3:.1f} [{min(tb) * 1e3:.1f}, {max(tb) * 1e3:.1f}] | {ml * 1e3:.1f} [{min(tl) * 1e3:.1f}, "
        f"{max(tl) * 1e3:.1f}] | {ml / mb:.2f} | {err:.1e} |")


def loop_over_times(p, name, x, times):
    """The loop of util.make_multi_time_argument: one single-time call per value, stacked along axis 1."""
    return np.stack([getattr(p, name)(x, time=float(t)) for t in times], axis=1)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "grad_multi_probe.txt")
    info = ctx.device_info()
    say(f"device: {info['arch']}, {info['n_cu']} CUs; {REPS} repetitions after one warm-up, variants alternating; "
        "ms, median [min, max]")
    d_state, m = 30, 2000
    x_all = bench.gaussian_mixture(500_000, d_state + 1, 4)
    x_all[:, -1] = np.repeat(np.arange(8.0), x_all.shape[0] // 8 + 1)[:x_all.shape[0]]
    rng = np.random.default_rng(4)
    c = np.ascontiguousarray(x_all[rng.choice(x_all.shape[0], m, replace=False)])
    ls = 0.5 * float(np.sqrt(((x_all[:2000, None, :d_state] - c[None, :50, :d_state]) ** 2).sum(-1)).mean())
    product = cov.Matern52(ls, active_dims=slice(None, -1)) * cov.Matern52(1.5, active_dims=-1)
    leaf = cov.Matern52(ls)

    say()
    say("predict_gradient, 100 000 x 2 000, one call with (m, p) weights against p calls with (m,) weights")
    say("| kernel, p | one call | p calls | loop / one call | max diff / max |")
    say("|---|---|---|---|---|")
    xq = np.ascontiguousarray(x_all[:100_000])
    for name, tree in (("Matern52 leaf", leaf), ("product", product)):
        desc = tree.lower(d_state + 1)
        for p in (2, 8, 64):
            W = rng.normal(size=(m, p))
            cols = [np.ascontiguousarray(W[:, q]) for q in range(p)]
            compare(f"{name}, p = {p}",
                    lambda: ctx.predict_gradient(desc, xq, c, W),
                    lambda: np.stack([ctx.predict_gradient(desc, xq, c, w) for w in cols], axis=1),
                    reps=REPS if p < 64 else 3)

    say()
    say("PredictorTime, multi_time = 200 points, product Matern52 (C4: 5e5 x (30 + time), 2 000 centres)")
    say("| method, queries | grid | loop over times | loop / grid | max diff / max |")
    say("|---|---|---|---|---|")
    pt = PredictorTime(product, c, rng.normal(size=m) / np.sqrt(m), -30.0, n_obs=x_all.shape[0])
    times = np.linspace(0.0, 7.0, 200)
    xs = np.ascontiguousarray(x_all[:, :-1])
    compare("mean, 500 000", lambda: pt.mean(xs, multi_time=times), lambda: loop_over_times(pt, "mean", xs, times), reps=3)
    xd = np.ascontiguousarray(xs[:100_000])
    compare("time_derivative, 100 000", lambda: pt.time_derivative(xd, multi_time=times),
            lambda: loop_over_times(pt, "time_derivative", xd, times), reps=3)
    xg = np.ascontiguousarray(xs[:20_000])
    compare("gradient, 20 000", lambda: pt.gradient(xg, multi_time=times), lambda: loop_over_times(pt, "gradient", xg, times),
            reps=3)
    xt = np.ascontiguousarray(xs[:300])
    compare("mean, 300 (a trajectory)", lambda: pt.mean(xt, multi_time=times),
            lambda: loop_over_times(pt, "mean", xt, times))
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
