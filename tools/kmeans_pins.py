"""Pin what ctx.kmeans computes on every path through the level driver (csrc/kmeans.hip), bit for bit.

One case per path, at the smallest shape that takes it.  For each: sha256 of the centres' bytes, n_iter and the inertia as a
hex float; for init="sklearn" also the sha256 of the seed indices.  The cluster sums are fixed-point and the seeding draws from
block sums, so two runs of one build give the same file; tests/golden/kmeans_pins.json is the output of the build BEFORE the
driver was split into stages, and tests/test_gpu_kmeans_pins.py replays the cases against it.

    python tools/kmeans_pins.py [--lib path/to/libmellon_hip.so] [--out pins.json]
"""
import os as _os; _os.environ.setdefault("MELLON_AMD_EXPERIMENTAL", "1")   # this tool turns experiment knobs (csrc/mln_options.h)
import argparse
import hashlib
import json
import sys

import numpy as np

sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))

KNOBS = ("MELLON_AMD_KM_LEVELS", "MELLON_AMD_KM_BOUNDS", "MELLON_AMD_KM_FP16", "MELLON_AMD_KM_PRUNE")
ONE_LEVEL = {"MELLON_AMD_KM_LEVELS": "1"}

# name -> (n, d, m, keyword arguments of ctx.kmeans, experiment knobs, pass the cells as a DeviceArray)
CASES = {
    "tiny":           (60, 3, 50, {}, ONE_LEVEL, False),                        # fp64 seeding, k_assign (n m < 4096)
    "mfma":           (5000, 12, 100, {}, ONE_LEVEL, False),                    # fp64 seeding, k_assign_mfma
    "wide":           (16384, 62, 1024, {"max_iter": 30}, ONE_LEVEL, False),    # prepared, fp64 seeding, unfolded fp16 sweep
    "hamerly":        (16384, 8, 1024, {"max_iter": 40}, ONE_LEVEL, False),     # fp16 seeding, folded sweep, Hamerly bounds
    "hamerly-device": (16384, 8, 1024, {"max_iter": 40}, ONE_LEVEL, True),      # the same from resident cells
    "seed-only":      (16384, 8, 1024, {"max_iter": 0}, ONE_LEVEL, False),      # seeding and download only
    "no-bounds":      (16384, 8, 1024, {"max_iter": 30}, {**ONE_LEVEL, "MELLON_AMD_KM_BOUNDS": "0"}, False),
    "no-fp16":        (16384, 8, 1024, {"max_iter": 10}, {**ONE_LEVEL, "MELLON_AMD_KM_FP16": "0"}, False),
    "groups":         (65536, 8, 1024, {"max_iter": 40}, ONE_LEVEL, False),     # group bounds at their threshold
    "groups-ragged":  (66000, 5, 1025, {"max_iter": 20}, ONE_LEVEL, False),     # a one-centre last stage, n % 256 != 0
    "two-level":      (262144, 8, 256, {}, {}, False),                          # coarse level, fine level Hamerly from init
    "sklearn":        (16384, 8, 1024, {"init": "sklearn", "max_iter": 20}, ONE_LEVEL, False),
    "sklearn-seeds":  (16384, 8, 1024, {"init": "sklearn", "max_iter": 0}, ONE_LEVEL, False),   # the copy-out branch
}


def case_input(name):
    from oracle import mellon_oracle as mo
    n, d = CASES[name][:2]
    x = mo.gaussian_mixture(n, d, seed=d + 1)
    if name != "tiny":
        x[100:120] = x[200:220]                    # exact duplicates
    return np.ascontiguousarray(x)


def run_case(ctx, name):
    n, d, m, kwargs, knobs, resident = CASES[name]
    x = case_input(name)
    saved = {k: _os.environ.pop(k, None) for k in KNOBS}
    _os.environ.update(knobs)
    try:
        centres, n_iter, inertia = ctx.kmeans(ctx.to_device(x) if resident else x, m, return_info=True, **kwargs)
    finally:
        for k, v in saved.items():
            _os.environ.pop(k, None)
            if v is not None:
                _os.environ[k] = v
    pin = {"centres": hashlib.sha256(np.ascontiguousarray(centres).tobytes()).hexdigest(), "n_iter": int(n_iter),
           "inertia": float(inertia).hex()}
    if kwargs.get("init") == "sklearn":
        pin["seed_indices"] = hashlib.sha256(np.ascontiguousarray(ctx.last_kmeans_seed_indices).tobytes()).hexdigest()
    return pin


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--lib", help="library to load instead of the tree's own build")
    ap.add_argument("--out", help="write the pins here (default: standard output)")
    args = ap.parse_args()
    from mellon_amd import _lib
    if args.lib:
        _lib.LIB_PATH = _os.path.abspath(args.lib)
    ctx = _lib.default_context()
    pins = {}
    for name in CASES:
        pins[name] = run_case(ctx, name)
        print(name, pins[name], file=sys.stderr, flush=True)
    text = json.dumps(pins, indent=1, sort_keys=True) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
