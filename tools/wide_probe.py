"""Cells with 65 to 256 features: the wide 1-NN route against the scalar fp64 search, and device k-means against sklearn's
(run by hand on the GPU box; writes profiles/wide_cells.txt, or the path given as the first argument).

1-NN     n = 262 144 cells of oracle-style Gaussian mixtures (bench.gaussian_mixture), d in {96, 128, 256}: the default route
         (MELLON_AMD_NN_PREFILTER unset: the wide sweep, csrc/rowmin_wide.hip) against MELLON_AMD_NN_PREFILTER=0 (the scalar
         fp64 kernel), one warm-up of each, then REPS timed calls with the two arms alternating in this process; the share
         of rows the certification left open and the largest relative difference of the two results.
         On a build without Context.nn_last (the parent commit) only the scalar arm exists and only it is timed: that run
         is the baseline the wide route is compared with.
k-means  (200 000, 128) cells, 2000 centres: Context.kmeans (one warm-up, REPS timed calls) against
         sklearn.cluster.k_means(n_init=1) on the same cells (host, minutes: timed once), and both inertias.
         --no-sklearn leaves the host arm out.

Every device call is synchronous (host arrays in and out), so the wall clock around it is what a caller waits for."""
import os
import sys
import time

sys.path.insert(0, ".")
import numpy as np

import bench
from mellon_amd import _lib

REPS = 3
N_NN = 262144
NN_DIMS = (96, 128, 256)
KM_SHAPE = (200000, 128, 2000)
ctx = _lib.default_context()
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


def with_env(key, value, f):
    old = os.environ.get(key)
    if value is None:
        os.environ.pop(key, None)
    else:
        os.environ[key] = value
    try:
        return f()
    finally:
        if old is None:
            os.environ.pop(key, None)
        else:
            os.environ[key] = old


def fmt(ts):
    return f"{np.median(ts) * 1e3:.1f} [{min(ts) * 1e3:.1f}, {max(ts) * 1e3:.1f}]"


def probe_nn(has_wide):
    say(f"1-NN, {N_NN} cells against themselves; ms, median [min, max] of {REPS} calls after one warm-up, arms alternating")
    say("| d | default route | route id | PREFILTER=0 (scalar fp64) | scalar / default | rows left open | max rel. diff |")
    say("|---|---|---|---|---|---|---|")
    for d in NN_DIMS:
        x = bench.gaussian_mixture(N_NN, d, d)
        scalar = lambda: with_env("MELLON_AMD_NN_PREFILTER", "0", lambda: ctx.nn_distances(x))
        default = lambda: with_env("MELLON_AMD_NN_PREFILTER", None, lambda: ctx.nn_distances(x))
        _, ref = timed(scalar)
        if not has_wide:
            ts = [timed(scalar)[0] for _ in range(REPS)]
            say(f"| {d} | - | - | {fmt(ts)} | - | - | - |")
            continue
        _, got = timed(default)
        last = ctx.nn_last()
        err = np.abs(got / ref - 1).max()
        td, ts = [], []
        for _ in range(REPS):
            td.append(timed(default)[0])
            ts.append(timed(scalar)[0])
        say(f"| {d} | {fmt(td)} | {int(last[0])} | {fmt(ts)} | {np.median(ts) / np.median(td):.1f} | "
            f"{int(last[1])} ({100.0 * last[1] / N_NN:.2f} %) | {err:.1e} |")
        assert err <= 1e-12, err
        del got
    say()


def probe_kmeans(run_sklearn):
    n, d, m = KM_SHAPE
    x = bench.gaussian_mixture(n, d, 7)
    say(f"k-means, {n} x {d} cells, {m} centres; device: ms, median [min, max] of {REPS} calls after one warm-up")
    try:
        _, (c, it, inertia) = timed(lambda: ctx.kmeans(x, m, seed=42, return_info=True))
    except _lib.MellonHipError as e:
        say(f"device k-means: refused ({e})")
        inertia = None
    if inertia is not None:
        ts = [timed(lambda: ctx.kmeans(x, m, seed=42))[0] for _ in range(REPS)]
        say(f"device k-means: {fmt(ts)} ms, {it} sweeps, inertia {inertia:.6e}")
    if run_sklearn:
        from sklearn.cluster import k_means
        say("sklearn.cluster.k_means(n_init=1, random_state=42): running (host, timed once) ...")
        t, (_, _, ref_inertia) = timed(lambda: k_means(x, m, n_init=1, random_state=42))
        say(f"sklearn k_means: {t:.1f} s, inertia {ref_inertia:.6e}")
        if inertia is not None:
            say(f"sklearn / device time: {t / np.median(ts):.0f}; device / sklearn inertia: {inertia / ref_inertia:.4f}")
    say()


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join("profiles", "wide_cells.txt")
    info = ctx.device_info()
    has_wide = hasattr(ctx, "nn_last")
    say("command: python tools/wide_probe.py" + ("" if has_wide else "   (build without the wide route: scalar arm only)"))
    say(f"device: {info['arch']}, {info['n_cu']} CUs")
    say()
    probe_nn(has_wide)
    if "--no-kmeans" not in sys.argv:
        probe_kmeans("--no-sklearn" not in sys.argv)
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
