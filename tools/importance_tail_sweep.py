"""The importance tail of the MAP solve (MELLON_AMD_IMPORTANCE_TAIL) on more than one seed and on data it was not tuned on:
the default fp64 fit with the tail on and off,

  * at C3 (1e6 x 50, 5000 landmarks, Matern52) over the data seeds of tools/solver_sweep.py's tables, and
  * on the generators of tools/robustness_sweep_large.py (tree d = 20 / 10, duplicates, heavy tails, two scales; 1e6 cells,
    2000 landmarks), three generator seeds each, so that the parent's own seed-to-seed spread is on the table.

Per fit: full passes, row-list passes, pass-equivalents, step ms (best of two), status, guard, distance from the tail-off fit.
    python tools/importance_tail_sweep.py [c3] [hard] [default] [n]        (on a GPU box)
"default": the "on" fits leave the switch unset, so the library's cost rule decides (otherwise the tail is forced on)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("MELLON_AMD_EXPERIMENTAL", "1")
os.environ["MELLON_AMD_MIXED"] = "0"
import numpy as np
import bench, mellon_amd
from mellon_amd import _lib

args = sys.argv[1:]
n = next((int(float(a)) for a in args if a[0].isdigit()), 1_000_000)
ON = "default" if "default" in args else "1"        # "on" column: the tail forced on, or the library's own cost rule
args = [a for a in args if a != "default"]
which = [a for a in args if not a[0].isdigit()] or ["c3", "hard"]
print(f"# 'on' = {'the default (cost rule decides)' if ON == 'default' else 'MELLON_AMD_IMPORTANCE_TAIL=1 (forced)'}; 'off' = MELLON_AMD_IMPORTANCE_TAIL=0", flush=True)
ctx = _lib.default_context()


def fit(xd, lm, nn, tail, kern=None):
    os.environ.pop("MELLON_AMD_IMPORTANCE_TAIL", None)
    if tail != "default":
        os.environ["MELLON_AMD_IMPORTANCE_TAIL"] = tail
    best = None
    for rep in range(2):
        kw = {"cov_func_curry": kern} if kern is not None else {}
        est = mellon_amd.DensityEstimator(landmarks=lm, nn_distances=nn, check_rank=False, **kw)
        ctx.synchronize(); t0 = time.perf_counter()
        dens = est.fit_predict(xd)
        dt = time.perf_counter() - t0
        st = est._fit.stage_times()
        status = int(getattr(est.opt_state, "status", -1))
        est._fit.close()
        if best is None or dt < best[0]:
            best = (dt, st, status)
    return dens, best


def row(tag, xd, lm, nn, kern=None):
    off, (dt0, s0, st0) = fit(xd, lm, nn, "0", kern)
    on, (dt1, s1, st1) = fit(xd, lm, nn, ON, kern)
    rel = float(np.abs(on - off).max() / np.abs(off).max())
    print(f"{tag:44s} off: {int(s0['objective_launches']):3d} full {s0['objective_pass_equivalents']:6.2f} pe {1e3 * dt0:7.1f} ms st {st0} rb {int(s0['precond_rebuilds'])} | "
          f"on: {int(s1['objective_launches']):3d} full {int(s1['objective_tail_launches']):3d} list {s1['objective_pass_equivalents']:6.2f} pe {1e3 * dt1:7.1f} ms st {st1} "
          f"rb {int(s1['precond_rebuilds'])} guard {int(s1['objective_tail_guard'])} | on vs off {rel:.1e}", flush=True)
    return s0["objective_pass_equivalents"], s1["objective_pass_equivalents"]


if "c3" in which:
    for seed in (3, 4, 5, 6, 7):
        x = bench.gaussian_mixture(n, 50, seed)
        lm, _ = bench.make_landmarks(x, 5000, "device", ctx)
        xd = ctx.to_device(x); nn = ctx.nn_distances(xd, xd)
        row(f"C3 seed {seed}", xd, lm, nn, mellon_amd.cov.Matern52)
        xd.free()

if "hard" in which:
    def trajectories(rng, n, d, branches=6):
        t = rng.beta(0.7, 1.3, size=n); b = rng.integers(0, branches, size=n)
        dirs = rng.normal(size=(branches, 3)); dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        bend = rng.normal(size=(branches, 3)) * 0.5
        z = t[:, None] * dirs[b] + (t ** 2)[:, None] * bend[b] + 0.02 * (1 + 3 * t)[:, None] * rng.normal(size=(n, 3))
        W1 = rng.normal(size=(3, d)); W2 = rng.normal(size=(3, d))
        x = np.tanh(z @ W1) + 0.3 * np.sin(2.0 * z @ W2)
        return np.ascontiguousarray(x * (0.8 ** np.arange(d))[None, :])

    def mixture(rng, n, d, k=10):
        means = rng.normal(0, 3, size=(k, d)); sig = rng.uniform(0.5, 1.5, size=k)
        c = rng.integers(0, k, size=n)
        return means[c] + rng.normal(size=(n, d)) * sig[c][:, None]

    def duplicated(rng, n):
        x = mixture(rng, n, 20); x[:n // 10] = x[n // 2:n // 2 + n // 10]; return x

    cases = {"tree d=20": lambda r: trajectories(r, n, 20), "tree d=10": lambda r: trajectories(r, n, 10),
             "mixture d=20, 10 % duplicates": lambda r: duplicated(r, n), "heavy tails t3 d=20": lambda r: r.standard_t(3, size=(n, 20)),
             "two scales d=20": lambda r: np.concatenate([0.01 * r.normal(size=(n // 20, 20)) + 4.0, mixture(r, n - n // 20, 20)])}
    for name, make in cases.items():
        offs, ons = [], []
        for seed in (11, 12, 13):
            x = np.ascontiguousarray(make(np.random.default_rng(seed)), dtype=np.float64)
            xd = ctx.to_device(x); nn = ctx.nn_distances(xd, xd)
            lm = ctx.kmeans(x[:100_000], 2000, seed=42)
            a, b = row(f"{name}, seed {seed}", xd, lm, nn)
            offs.append(a); ons.append(b)
            xd.free()
        print(f"{name:44s} pass-equivalents off {min(offs):.1f}..{max(offs):.1f} (spread {max(offs) - min(offs):.1f}) | on {min(ons):.1f}..{max(ons):.1f} | "
              f"worst on - off {max(b - a for a, b in zip(offs, ons)):+.1f}", flush=True)
