"""The landmark conditional on sparse (CSR) targets against the same numbers dense (run by hand on the GPU box):

  n = 2e5 cells, d = 20, p = 2000 outputs, m in {1000, 5000} landmarks, density in {0.02, 0.05, 0.10}
    dense    Context.sparse_solve(desc, x, xu, Y.toarray(), ...)       mln_sparse_solve, the unchanged dense route
    sparse   Context.sparse_solve_csr(desc, x, xu, CSRTargets, ...)    mln_sparse_solve_csr: row panels of y - mu built in HBM

Host arrays in, weights out on both sides (the dense array and the CSR holder are made before the clock starts: what is timed
is what a caller with the data in that form waits for).  One warm-up of each variant, then --reps timed repetitions with the
two variants alternating; median and [min, max] of the wall clock around the synchronous calls.  One JSON line per shape goes
to --out (profiles/sparse_targets_probe.jsonl), the table rows to stdout.

  --kernel-share DIR   additionally runs the sparse call alone under `rocprofv3 --kernel-trace --stats` (a child process of
                       its own, output under DIR) at each m and the middle density, and reports the share of k_csr_panel and
                       of the per-panel k_sum_partials in the kernel time of the call.
  --child M DENSITY    (used by --kernel-share) warm-up + 3 sparse calls of one shape, nothing else."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from mellon_amd import _lib, cov
from mellon_amd.validation import CSRTargets

D, LS, SIGMA, JITTER = 20, 6.0, 0.5, 1e-6


def make_inputs(n, m, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, D))
    xu = x[rng.choice(n, m, replace=False)] + 0.05 * rng.normal(size=(m, D))
    return x, xu


def make_targets(n, p, density, seed=1, rows_per_chunk=20000):
    """Random CSR targets built in row chunks (no n x p array): Bernoulli(density) pattern, standard normal values."""
    rng = np.random.default_rng(seed)
    counts, cols = [], []
    for r0 in range(0, n, rows_per_chunk):
        mask = rng.random((min(rows_per_chunk, n - r0), p)) < density
        counts.append(mask.sum(axis=1))
        cols.append(np.nonzero(mask)[1].astype(np.int32))
    indices = np.concatenate(cols)
    indptr = np.concatenate(([0], np.cumsum(np.concatenate(counts)))).astype(np.int64)
    return CSRTargets(indptr, indices, rng.standard_normal(indices.shape[0]), (n, p))


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


def stats(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts))}


def kernel_share(out_dir, n, p, m, density):
    """Kernel times of the sparse call from a rocprofv3 run of its own."""
    tag = f"m{m}_d{density}"
    d = os.path.join(out_dir, tag)
    os.makedirs(d, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
           os.path.abspath(__file__), "--n", str(n), "--p", str(p), "--child", str(m), str(density)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"rocprofv3 run failed ({r.returncode}): {r.stderr[-2000:]}")
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise RuntimeError(f"no kernel_stats.csv under {d}")
    total, by_name = 0.0, {}
    for row in csv.DictReader(open(files[0])):
        name = row.get("Name") or row.get("KernelName") or ""
        ns = float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0.0)
        total += ns
        for key in ("k_csr_panel", "k_sum_partials", "k_dgemm"):
            if key in name:
                by_name[key] = by_name.get(key, 0.0) + ns
    return {"kernel_time_total_ms": total / 1e6, **{k + "_ms": v / 1e6 for k, v in by_name.items()},
            **{k + "_share": v / total for k, v in by_name.items() if total > 0}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200_000)
    ap.add_argument("--p", type=int, default=2000)
    ap.add_argument("--m", type=int, nargs="+", default=[1000, 5000])
    ap.add_argument("--density", type=float, nargs="+", default=[0.02, 0.05, 0.10])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mu", type=float, default=0.0)
    ap.add_argument("--out", default="profiles/sparse_targets_probe.jsonl")
    ap.add_argument("--kernel-share", default=None, metavar="DIR")
    ap.add_argument("--child", nargs=2, default=None, metavar=("M", "DENSITY"))
    a = ap.parse_args()
    ctx = _lib.default_context()
    if a.child:
        m, density = int(a.child[0]), float(a.child[1])
        x, xu = make_inputs(a.n, m)
        y = make_targets(a.n, a.p, density)
        desc = cov.Matern52(LS).lower(D)
        for _ in range(4):
            ctx.sparse_solve_csr(desc, x, xu, y, a.mu, SIGMA, ctx.SIGMA_SCALAR, JITTER)
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    info = ctx.device_info()
    print(f"device {info['arch']}, {info['n_cu']} CUs; n = {a.n}, d = {D}, p = {a.p}, mu = {a.mu}, CSR panel "
          f"{_lib.CSR_PANEL_BYTES >> 20} MiB = {_lib.csr_panel_rows(a.p)} rows; {a.reps} repetitions, median [min, max] in ms")
    print("| m | density | nnz | dense y | sparse y | sparse / dense | 1 + 70 / m | max rel. difference |")
    print("|---|---|---|---|---|---|---|---|")
    desc = cov.Matern52(LS).lower(D)
    with open(a.out, "w") as out:
        for density in a.density:
            y = make_targets(a.n, a.p, density)
            yd = y.toarray()
            for m in a.m:
                x, xu = make_inputs(a.n, m)
                dense = lambda: ctx.sparse_solve(desc, x, xu, yd, a.mu, SIGMA, JITTER)
                sparse = lambda: ctx.sparse_solve_csr(desc, x, xu, y, a.mu, SIGMA, ctx.SIGMA_SCALAR, JITTER)
                wd, ws = timed(dense)[1], timed(sparse)[1]           # warm-up of both, and the comparison of the results
                err = float(np.abs(ws - wd).max() / np.abs(wd).max())
                del wd, ws
                td, ts = [], []
                for _ in range(a.reps):
                    td.append(timed(dense)[0])
                    ts.append(timed(sparse)[0])
                rec = {"n": a.n, "d": D, "p": a.p, "m": m, "density": density, "nnz": y.nnz, "mu": a.mu, "reps": a.reps,
                       "panel_bytes": _lib.CSR_PANEL_BYTES, "panel_rows": _lib.csr_panel_rows(a.p), "dense": stats(td),
                       "sparse": stats(ts), "ratio_median": float(np.median(ts) / np.median(td)),
                       "derived_ratio": 1.0 + 70.0 / m, "rel_max_sparse_vs_dense": err, "arch": info["arch"]}
                if a.kernel_share and density == sorted(a.density)[len(a.density) // 2]:
                    rec["kernels"] = kernel_share(a.kernel_share, a.n, a.p, m, density)
                out.write(json.dumps(rec) + "\n")
                out.flush()
                f = lambda s: f"{s['median_s'] * 1e3:.0f} [{s['min_s'] * 1e3:.0f}, {s['max_s'] * 1e3:.0f}]"
                print(f"| {m} | {density} | {y.nnz} | {f(rec['dense'])} | {f(rec['sparse'])} | {rec['ratio_median']:.3f} | "
                      f"{rec['derived_ratio']:.3f} | {err:.1e} |", flush=True)
                if "kernels" in rec:
                    print("  kernels of the sparse call:", json.dumps(rec["kernels"]), flush=True)
            del yd


if __name__ == "__main__":
    main()
