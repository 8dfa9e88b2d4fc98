"""Wall time of the block-evaluated derivatives (mellon_amd/block_derivatives.py) next to the one-program route:
predict_gradient / predict_hessian of the six-leaf sum of products and of a single Matern52 at n queries x m centres.
Every call is synchronous on return; each shape is warmed up once, then timed `--reps` times (median and range printed).

    python tools/time_block_derivatives.py [--n 100000] [--m 5000] [--d 4] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def six_leaf(c):
    return (c.Matern52(1.5, active_dims=[0, 1]) * c.ExpQuad(2.5, active_dims=[2, 3])
            + c.Matern32(1.1, active_dims=[0, 2]) * c.Exponential(3.0, active_dims=[1, 3])
            + 0.5 * (c.RatQuad(2.0, 1.7, active_dims=[1, 2]) * c.ExpQuad(1.9, active_dims=[0, 3])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--m", type=int, default=5000)
    ap.add_argument("--d", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    from mellon_amd import _lib, cov
    ctx = _lib.default_context()
    rng = np.random.default_rng(0)
    x, c, w = rng.normal(size=(args.n, args.d)), rng.normal(size=(args.m, args.d)), rng.normal(size=args.m)
    cases = {"six_leaf (block-evaluated)": six_leaf(cov).lower(args.d), "Matern52 (one program)": cov.Matern52(2.0).lower(args.d)}
    out = {"n": args.n, "m": args.m, "d": args.d, "reps": args.reps}
    for name, desc in cases.items():
        for what, fn in (("gradient", ctx.predict_gradient), ("hessian", ctx.predict_hessian)):
            fn(desc, x, c, w)                                # warm-up: code objects, the allocator's cache
            times = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                fn(desc, x, c, w)
                times.append(time.perf_counter() - t0)
            out[f"{name} {what}"] = {"median_s": float(np.median(times)), "min_s": min(times), "max_s": max(times)}
            print(f"{name:30s} {what:9s} median {np.median(times):8.4f} s  (min {min(times):.4f}, max {max(times):.4f})", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
