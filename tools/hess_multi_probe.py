"""One multi-output / fused device call against the loop it replaces (run by hand on the GPU box):

  * Context.predict_hessian with (m, p) weights against p single-output calls, p in {2, 8, 64}, Matern52 leaf, 2 000 centres,
    d = 5 and d = 30.  100 000 queries where the (n, p, d, d) result stays within RESULT_DOUBLES (2 GiB of host memory);
    fewer otherwise -- the row says how many;
  * Predictor.hessian_log_determinant (the fused entry) against np.linalg.slogdet(Predictor.hessian(x)), the host path,
    at 1e6 queries x 30 columns x 2 000 centres;
  * PredictorTime.hessian / hessian_log_determinant with multi_time = 50 points through the grid path against the per-time loop
    of util.make_multi_time_argument, product Matern52 at the C4 columns of BASELINE.md (30 + time, 2 000 centres, ls_time =
    1.5): the Hessian on as many of the queries as keep (n, 50, 30, 30) within RESULT_DOUBLES, the log-determinant on 100 000.

Host arrays in and out on both sides, so every figure is what a caller of the Python API waits for.  One warm-up of each
variant, then REPS timed repetitions with the two variants alternating; median and [min, max] of the wall clock around the
synchronous calls.  Writes the table to profiles/hess_multi_probe.txt (or the path given as the first argument)."""
import os
import sys
import time

sys.path.insert(0, ".")
import numpy as np

import bench
from mellon_amd import _lib, cov
from mellon_amd.base_predictor import Predictor, PredictorTime

REPS = 3
RESULT_DOUBLES = 1 << 28
ctx = _lib.default_context()
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


def diff(a, b):
    """max |a - b| / max |b|; for (sign, logabsdet) pairs: the largest |difference of logabsdet|, 'signs differ' if they do."""
    if isinstance(a, tuple):
        if not np.array_equal(a[0], b[0]):
            return "signs differ"
        return f"{np.abs(a[1] - b[1]).max():.1e} (abs)"
    return f"{np.abs(a - b).max() / max(np.abs(b).max(), 1e-300):.1e}"


def compare(label, batched, loop, reps=REPS):
    """Alternate the two variants; prints one table row."""
    _, a = timed(batched)
    _, b = timed(loop)
    err = diff(a, b)
    del a, b
    tb, tl = [], []
    for _ in range(reps):
        tb.append(timed(batched)[0])
        tl.append(timed(loop)[0])
    mb, ml = np.median(tb), np.median(tl)
    say(f"| {label} | {mb * 1e3:.1f} [{min(tb) * 1e3:.1f}, {max(tb) * 1e3:.1f}] | {ml * 1e3:.1f} [{min(tl) * 1e3:.1f}, "
        f"{max(tl) * 1e3:.1f}] | {ml / mb:.2f} | {err} |")


def loop_over_times(p, name, x, times):
    """The loop of util.make_multi_time_argument: one single-time call per value, stacked along axis 1."""
    outs = [getattr(p, name)(x, time=float(t)) for t in times]
    if isinstance(outs[0], tuple):
        return tuple(np.stack([o[k] for o in outs], axis=1) for k in range(2))
    return np.stack(outs, axis=1)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "hess_multi_probe.txt")
    info = ctx.device_info()
    say("command: python tools/hess_multi_probe.py")
    say(f"device: {info['arch']}, {info['n_cu']} CUs; {REPS} repetitions after one warm-up, variants alternating; "
        "ms, median [min, max]")
    d_state, m = 30, 2000
    x_all = bench.gaussian_mixture(1_000_000, d_state + 1, 4)
    x_all[:, -1] = np.repeat(np.arange(8.0), x_all.shape[0] // 8 + 1)[:x_all.shape[0]]
    rng = np.random.default_rng(4)
    c_all = np.ascontiguousarray(x_all[rng.choice(x_all.shape[0], m, replace=False)])

    def length_scale(d):
        return 0.5 * float(np.sqrt(((x_all[:2000, None, :d] - c_all[None, :50, :d]) ** 2).sum(-1)).mean())

    say()
    say("predict_hessian, n x 2 000, Matern52 leaf, one call with (m, p) weights against p calls with (m,) weights")
    say("| d, p, queries | one call | p calls | loop / one call | max diff / max |")
    say("|---|---|---|---|---|")
    for d in (5, 30):
        desc = cov.Matern52(length_scale(d)).lower(d)
        c = np.ascontiguousarray(c_all[:, :d])
        for p in (2, 8, 64):
            n = min(100_000, RESULT_DOUBLES // (p * d * d) // 1000 * 1000)
            xq = np.ascontiguousarray(x_all[:n, :d])
            W = rng.normal(size=(m, p))
            cols = [np.ascontiguousarray(W[:, q]) for q in range(p)]
            compare(f"d = {d}, p = {p}, {n}",
                    lambda: ctx.predict_hessian(desc, xq, c, W),
                    lambda: np.stack([ctx.predict_hessian(desc, xq, c, w) for w in cols], axis=1))

    say()
    say("Predictor.hessian_log_determinant, Matern52 leaf, 1 000 000 x 30, 2 000 centres: fused entry against slogdet(hessian(x))")
    say("| queries | fused | host path | host / fused | max diff of logabsdet |")
    say("|---|---|---|---|---|")
    d = d_state
    pred = Predictor(cov.Matern52(length_scale(d)), np.ascontiguousarray(c_all[:, :d]), rng.normal(size=m) / np.sqrt(m), -30.0)
    xq = np.ascontiguousarray(x_all[:, :d])
    compare("1 000 000", lambda: pred.hessian_log_determinant(xq), lambda: tuple(np.linalg.slogdet(pred.hessian(xq))), reps=2)
    del xq

    say()
    say("PredictorTime, multi_time = 50 points, product Matern52 (30 + time columns, 2 000 centres): grid against the loop")
    say("| method, queries | grid | loop over times | loop / grid | max diff |")
    say("|---|---|---|---|---|")
    product = cov.Matern52(length_scale(d_state), active_dims=slice(None, -1)) * cov.Matern52(1.5, active_dims=-1)
    pt = PredictorTime(product, c_all, rng.normal(size=m) / np.sqrt(m), -30.0, n_obs=x_all.shape[0])
    times = np.linspace(0.0, 7.0, 50)
    n = RESULT_DOUBLES // (50 * (d_state + 1) ** 2) // 1000 * 1000
    xh = np.ascontiguousarray(x_all[:n, :-1])
    compare(f"hessian, {n}", lambda: pt.hessian(xh, multi_time=times), lambda: loop_over_times(pt, "hessian", xh, times))
    xl = np.ascontiguousarray(x_all[:100_000, :-1])
    compare("hessian_log_determinant, 100 000", lambda: pt.hessian_log_determinant(xl, multi_time=times),
            lambda: loop_over_times(pt, "hessian_log_determinant", xl, times), reps=2)
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
