"""Extended-precision restatement of the predictive mean mu + cov(x, centres) w (reference conditional.py:899-906) with
the kernel formulas as oracle/mellon_oracle.py states them, the input recipe of the predictive-mean tests and their
per-row error bound.  Everything is np.longdouble and squared distances come from direct differences, so the reference
shares neither the xx - 2 xy + yy cancellation nor the summation order of the device.  Test infrastructure only: the
product never imports it."""
import numpy as np

LD = np.longdouble
KINDS = ("Matern32", "Matern52", "ExpQuad", "Exponential", "RatQuad", "Linear")
CO_RADIUS = 0.05          # pairs closer than this are "coincident": the cancellation of the float64 distance sets their error
ROW_CHUNK = 256           # rows per block of the distance loop (a block of longdouble pairs stays in cache)


def _select(a, active_dims):
    """oracle select_active_dims (util.py:150-171): None, a scalar, a slice, an index list or a boolean mask."""
    a = np.asarray(a, dtype=np.float64)
    a = a.reshape(a.shape[0], -1)
    if active_dims is None:
        return a
    if np.isscalar(active_dims):
        active_dims = [active_dims]
    return a[:, active_dims]


def kernel_ref(kind, params, x, y, active_dims=None):
    """(K, dist) in longdouble: dist = sqrt(sum_k (x_ik - y_jk)^2 + 1e-12) (oracle distance: the 1e-12 inside the root),
    K the kernel formula of the oracle.  params: ls, or (alpha, ls) for RatQuad (the oracle's argument order)."""
    xs, ys = _select(x, active_dims).astype(LD), _select(y, active_dims).astype(LD)
    n, m, d = xs.shape[0], ys.shape[0], xs.shape[1]
    assert ys.shape[1] == d
    if kind == "RatQuad":
        alpha, ls = (LD(p) for p in params)
    else:
        ls = LD(params[0] if isinstance(params, (tuple, list)) else params)
    sq, dot = np.zeros((n, m), dtype=LD), np.zeros((n, m), dtype=LD)
    t = np.empty((min(ROW_CHUNK, n), m), dtype=LD)
    for i0 in range(0, n, ROW_CHUNK):
        xc = xs[i0:i0 + ROW_CHUNK]
        tc, sc, dc = t[:xc.shape[0]], sq[i0:i0 + ROW_CHUNK], dot[i0:i0 + ROW_CHUNK]
        for k in range(d):
            if kind == "Linear":
                np.multiply(xc[:, k, None], ys[None, :, k], out=tc)
                dc += tc
            np.subtract(xc[:, k, None], ys[None, :, k], out=tc)
            np.multiply(tc, tc, out=tc)
            sc += tc
    dist = np.sqrt(sq + LD(1e-12))
    if kind == "Matern32":
        r = np.sqrt(LD(3)) * dist / ls
        K = (r + 1) * np.exp(-r)
    elif kind == "Matern52":
        r = np.sqrt(LD(5)) * dist / ls
        K = (r + np.square(r) / 3 + 1) * np.exp(-r)
    elif kind == "ExpQuad":
        K = np.exp(-np.square(dist / ls) / 2)
    elif kind == "Exponential":
        K = np.exp(-(dist / ls) / 2)                      # (the reference's non-standard / 2)
    elif kind == "RatQuad":
        K = (np.square(dist / ls) / (2 * alpha) + 1) ** -alpha
    elif kind == "Linear":
        K = dot / ls
    else:
        raise ValueError(kind)
    return K, dist


def mean_of(K, w, mu):
    """(mean, absdot) of a longdouble kernel matrix: mu + sum_j K_ij w_j and sum_j |K_ij w_j|, summed in longdouble."""
    P = K * np.asarray(w, dtype=np.float64).astype(LD)[None, :]
    return LD(mu) + P.sum(axis=1), np.abs(P).sum(axis=1)


def predict_mean_ref(kind, params, x, y, w, mu, active_dims=None):
    """(mean, absdot, K, dist): the longdouble mean and sum_j |K_ij w_j|, the float64 rounding of the longdouble kernel
    matrix, and the pair distances."""
    K, dist = kernel_ref(kind, params, x, y, active_dims)
    mean, absdot = mean_of(K, w, mu)
    return mean, absdot, K.astype(np.float64), dist


def length_scale(d):
    """Typical pair distances of a few length scales at every d (test_kernel_matrix_persistent_rows)."""
    return 1.7 * np.sqrt(max(d, 8) / 8.0)


def kind_params(kind, d):
    return (2.0, length_scale(d)) if kind == "RatQuad" else (length_scale(d),)


def recipe_counts(n):
    """(coincident, far, near) counts: 100 / 60 / 50 from 4096 cells on -- 2.4 % coincident and 1.2 % near-coincident
    rows -- and the same shares, at least one each, of fewer cells."""
    if n >= 4096:
        return 100, 60, 50
    return max(1, 100 * n // 4096), max(1, 60 * n // 4096), max(1, 50 * n // 4096)


def make_inputs(n, m, d, seed, counts=None):
    """The recipe of test_kernel_matrix_persistent_rows at any shape: x, y ~ 1.5 N(0, 1); the first h centres ARE cells
    (the +1e-12 branch); `far` cells scaled by 400 (e^-r underflows, RatQuad's tail does not); the last `near` centres lie
    1e-3 from cells that are neither; w ~ N(0, 1)."""
    h, far, near = counts or recipe_counts(n)
    assert h + near <= m and h + far + near <= n
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, d)) * 1.5
    y = rng.normal(size=(m, d)) * 1.5
    w = rng.normal(size=m)
    y[:h] = x[:h]
    x[h:h + far] *= 400.0
    y[m - near:] = x[h + far:h + far + near] + 1e-3 * rng.normal(size=(near, d))
    return x, y, w


def pair_tolerance(K, dist, tolK, tolCo):
    """Per-pair tolerance of a kernel value: tolK, or tolCo at pairs closer than CO_RADIUS, relative to the largest
    |K| of the row where that exceeds 1 (Linear, sums and scaled kernels; 1 for every stationary kind).  Also returns
    the coincident mask."""
    co = np.asarray(dist < CO_RADIUS)
    scale = np.maximum(1.0, np.abs(np.asarray(K, dtype=np.float64)).max(axis=1))[:, None]
    return np.where(co, tolCo, tolK) * scale, co


def row_bound(K, dist, w, absdot, tolK, tolCo):
    """tolK sum_{j not in co(i)} |w_j| + tolCo sum_{j in co(i)} |w_j| + (m + 64) 2^-53 absdot_i: the kernel values'
    tolerances times their weights, plus the standard bound of a length-m floating-point sum in any order."""
    tol, _ = pair_tolerance(K, dist, tolK, tolCo)
    m = tol.shape[1]
    return tol @ np.abs(np.asarray(w, dtype=np.float64)) + (m + 64) * 2.0 ** -53 * np.asarray(absdot, dtype=np.float64)
