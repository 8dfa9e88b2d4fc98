"""Record what the predictor gradient / Hessian routes return, bit for bit (run by hand on the GPU box):

    python tools/deriv_routes_dump.py [tests/golden/deriv_routes_parent.npz]

Seeded inputs; Context.predict_gradient, Context.predict_hessian and Context.predict_hessian_logdet (lead = d) for every tree of
_trees(d) of tests/test_gpu_predict_gradient_multi.py on the shapes of cases(): the smallest call, the per-column route, the
GEMM routes (single-output and batched, ragged tiles), the row-chunk seams of the gradient and of the Hessian launchers, and
the GEMM / seam shapes again with one output per block.  (m, p) weights everywhere; for p == 1 the (m,) form as well.

Only outputs are written: one flat float64 array `data` and a JSON `index`, name -> [offset, shape].  Outputs with identical
bits (the (m,) and (m, 1) forms; a block size that does not change the sums) share one stretch of `data`.
tests/test_gpu_deriv_routes_pinned.py recomputes every output through outputs() below and compares it with the file."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "deriv_routes_parent.npz")
GRAD_SEAM, HESS_SEAM, SEAM_HALO = 32768, 16384, 64      # rows per chunk of the gradient / Hessian launchers at m = 64
ONE_BLOCK_ENV = ("MELLON_AMD_GRAD_COLS", "MELLON_AMD_HESS_COLS")   # "1": fewer columns than one output has, P_b = 1


def cases():
    """key -> (n, m, d, p, rows stored, entries called, one output per block)"""
    both, all_rows = ("grad", "hess"), slice(None)
    out = {"tiny": (1, 1, 1, 1, all_rows, both, False), "percol": (20, 30, 3, 4, all_rows, both, False)}
    for one in (False, True):
        tag = "_oneblock" if one else ""
        for p in (1, 2):
            out[f"gemm_p{p}{tag}"] = (130, 520, 3, p, all_rows, both, one)
            out[f"gradseam_p{p}{tag}"] = (GRAD_SEAM + 37, 64, 2, p, slice(GRAD_SEAM - SEAM_HALO, GRAD_SEAM + SEAM_HALO),
                                          ("grad",), one)
            out[f"hessseam_p{p}{tag}"] = (HESS_SEAM + 37, 64, 2, p, slice(HESS_SEAM - SEAM_HALO, HESS_SEAM + SEAM_HALO),
                                          ("hess",), one)
    return out


def outputs(ctx, key):
    """name -> array: every output of one case, cut to the rows the case stores."""
    if os.path.join(ROOT, "tests") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_predict_gradient_multi import _trees
    n, m, d, p, rows, entries, one = cases()[key]
    rng = np.random.default_rng([n, m, d, p])
    xq, c, W = rng.normal(size=(n, d)), rng.normal(size=(m, d)), rng.normal(size=(m, p))
    forms = {"2d": W} if p > 1 else {"2d": W, "1d": np.ascontiguousarray(W[:, 0])}
    saved = {e: os.environ.get(e) for e in ONE_BLOCK_ENV}
    for e in ONE_BLOCK_ENV:
        if one:
            os.environ[e] = "1"
        else:
            os.environ.pop(e, None)
    res = {}
    try:
        for tree, k in _trees(d).items():
            desc = k.lower(d)
            for form, w in forms.items():
                if "grad" in entries:
                    res[f"{key}/{tree}/grad_{form}"] = ctx.predict_gradient(desc, xq, c, w)[rows]
                if "hess" in entries:
                    res[f"{key}/{tree}/hess_{form}"] = ctx.predict_hessian(desc, xq, c, w)[rows]
                    sign, logabs = ctx.predict_hessian_logdet(desc, xq, c, w, lead=d)
                    res[f"{key}/{tree}/sign_{form}"], res[f"{key}/{tree}/logabs_{form}"] = sign[rows], logabs[rows]
    finally:
        for e, v in saved.items():
            if v is None:
                os.environ.pop(e, None)
            else:
                os.environ[e] = v
    return res


def load(path=FIXTURE):
    """name -> array from a file written by main()."""
    with np.load(path) as f:
        data, index = f["data"], json.loads(str(f["index"]))
    return {name: data[off:off + int(np.prod(shape, dtype=np.int64))].reshape(shape) for name, (off, shape) in index.items()}


def main():
    os.environ.setdefault("MELLON_AMD_EXPERIMENTAL", "1")     # as tests/conftest.py sets it
    sys.path.insert(0, ROOT)
    from mellon_amd import _lib
    ctx = _lib.default_context()
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    chunks, index, seen, size = [], {}, {}, 0
    for key in cases():
        for name, a in outputs(ctx, key).items():
            flat = np.ascontiguousarray(a, dtype=np.float64).ravel()
            off = seen.get(flat.tobytes())
            if off is None:
                off = seen[flat.tobytes()] = size
                chunks.append(flat)
                size += flat.size
            index[name] = [off, list(a.shape)]
        print(f"{key}: {size} doubles so far", flush=True)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    np.savez_compressed(path, data=np.concatenate(chunks), index=np.array(json.dumps(index)))
    print(f"{path}: {len(index)} outputs, {size} doubles, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
