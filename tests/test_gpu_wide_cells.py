"""Cells with 65 to 256 features on a real MI355X (-m gpu): the chunked fp16-split row-minimum sweep (csrc/rowmin_wide.hip), its
error bound, the exact 1-NN search and the k-means tier built on it, and the default estimator call on such cells."""
import functools
import logging

import numpy as np
import pytest

from oracle import mellon_oracle as mo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mellon():
    import mellon_amd
    return mellon_amd


@pytest.fixture(scope="module")
def ctx():
    from mellon_amd import _lib
    return _lib.default_context()


# ---- 1. the bound holds -------------------------------------------------------------------------------------------------
def _stress_rows(d):
    """2800 mixture rows, the first 1500 the queries and the last 1300 the candidates: a tight cluster far out in both
    parts, exact duplicates and rows 1e-9 apart inside the queries and across the two parts, one column in units of 1e-7."""
    rng = np.random.default_rng(1000 + d)
    z = mo.gaussian_mixture(2800, d, seed=d)
    z[:150] = 40.0 + 1e-3 * rng.normal(size=(150, d))
    z[1500:1650] = 40.0 + 1e-3 * rng.normal(size=(150, d))
    z[300:305] = z[310:315]
    z[1700:1705] = z[200:205]
    z[320:325] = z[330:335] + 1e-9
    z[1710:1715] = z[210:215] + 1e-9
    z[:, 1] *= 1e-7
    return np.ascontiguousarray(z[:1500]), np.ascontiguousarray(z[1500:])


@pytest.mark.parametrize("same", [False, True])
@pytest.mark.parametrize("d", [65, 67, 125, 126, 128, 129, 192, 253, 256])
def test_wide_sweep_values_lie_within_the_bound(ctx, d, same):
    """|approximate - exact| <= E for the winner, and no exact value lies below m1 - E, none but the winner's below m2 - E:
    the premise of the certificate, in the sweep's own centred and scaled units -- 1500 queries against 1300 candidates
    (rows and last stage ragged), every chunk count, both sides of each multiple of 64."""
    x, y = _stress_rows(d)
    if same:
        y = x
        m1, m2, arg, E, prep = ctx.diag_rowmin_wide(x, exclude_self=True, self_offset=0)
    else:
        m1, m2, arg, E, prep = ctx.diag_rowmin_wide(x, y)
    n, m = x.shape[0], y.shape[0]
    assert prep.shape == (d + 2,) and prep[d] > 0 and np.log2(prep[d]) == np.round(np.log2(prep[d]))
    xs, ys = (x - prep[:d]) * prep[d], (y - prep[:d]) * prep[d]
    assert 2.0**12 <= max((xs * xs).sum(1).max(), (ys * ys).sum(1).max()) < 2.0**14
    s = (ys * ys).sum(1)[None, :] - 2.0 * xs @ ys.T
    rows = np.arange(n)
    assert np.all(np.isfinite(E)) and np.all(E > 0)
    assert arg.min() >= 0 and arg.max() < m
    if same:
        assert np.all(arg != rows)
        s[rows, rows] = np.inf
    m1, m2 = m1.astype(np.float64), m2.astype(np.float64)
    assert np.all(np.abs(m1 - s[rows, arg]) <= E)
    assert np.all(s.min(1) >= m1 - E)
    others = s.copy()
    others[rows, arg] = np.inf
    assert np.all(others.min(1) >= m2 - E)
    assert np.all(m2 >= m1)


# ---- 2. exact 1-NN ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [65, 126, 128, 129, 256])
def test_wide_nn_exact(ctx, monkeypatch, d):
    """test_nn_prefilter_exact (tests/test_gpu_round3.py) for wide cells: the same construction, assertions and numbers; the
    pre-filtered call takes the wide route, the plain one the scalar fp64 kernel."""
    rng = np.random.default_rng(100 + d)
    n = 12000
    x = mo.gaussian_mixture(n, d, seed=d)
    x[:3000] = 40.0 + 1e-3 * rng.normal(size=(3000, d))
    x[3000:3010] = x[3010:3020]
    x[3020:3030] = x[3030:3040] + 1e-9
    want = mo.exact_nn_distances(x)
    monkeypatch.setenv("MELLON_AMD_NN_PREFILTER_MIN", "1")
    monkeypatch.setenv("MELLON_AMD_NN_PREFILTER", "1")
    fast = ctx.nn_distances(x)
    assert ctx.nn_last()[0] == 4
    monkeypatch.setenv("MELLON_AMD_NN_PREFILTER", "0")
    plain = ctx.nn_distances(x)
    assert ctx.nn_last()[0] == 0
    scale = np.linalg.norm(x, axis=1).max()
    tol2 = 64 * np.finfo(float).eps * scale**2
    assert np.abs(fast**2 - want**2).max() < tol2 and np.abs(plain**2 - want**2).max() < tol2
    assert np.all(fast[3000:3020] == 0) and np.all(plain[3000:3020] == 0) and np.all(want[3000:3020] == 0)
    assert np.allclose(fast[3020:3040], want[3020:3040], rtol=1e-9, atol=0)
    assert np.abs(fast[3040:] / want[3040:] - 1).max() < 1e-12 and np.abs(plain[3040:] / want[3040:] - 1).max() < 1e-12
    monkeypatch.setenv("MELLON_AMD_NN_PREFILTER", "1")
    lo, hi = 5000, 9000
    part = ctx.nn_distances(np.ascontiguousarray(x[lo:hi]), x, self_offset=lo)
    assert ctx.nn_last()[0] == 4
    assert np.array_equal(part, fast[lo:hi])
    lm = x[::37]
    from sklearn.neighbors import BallTree
    near = BallTree(lm).query(x[1::2], k=1)[0][:, 0]
    got = ctx.nn_distances(np.ascontiguousarray(x[1::2]), lm, self_offset=-n)        # i - n < 0: no pair excluded
    assert ctx.nn_last()[0] == 4
    assert np.abs(got**2 - near**2).max() < tol2


def test_wide_nn_is_not_pruned_at_the_pruned_size(ctx, monkeypatch):
    """2^18 + 17 cells against themselves is where narrow cells take the pruned search: wide cells take the wide route."""
    n, d = 2**18 + 17, 65
    x = mo.gaussian_mixture(n, d, seed=5)
    monkeypatch.setenv("MELLON_AMD_NN_PREFILTER", "1")
    fast = ctx.nn_distances(x)
    last = ctx.nn_last()
    assert last[0] == 4 and last[1] == last[2] and last[1] < n
    monkeypatch.setenv("MELLON_AMD_NN_PREFILTER", "0")
    plain = ctx.nn_distances(x)
    assert ctx.nn_last()[0] == 0
    assert np.abs(fast / plain - 1).max() < 1e-12


# ---- 3. the certificate decides most rows ---------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [65, 128, 256])
def test_wide_certificate_leaves_few_rows_open(ctx, monkeypatch, d):
    """At most a quarter of the rows of a plain mixture go to the exact re-search (with the narrow bound's terms scaled by the
    chunk count 1.7 % / 4.0 % / 8.4 % of these rows have their runner-up within 2 E): a bound loose enough to be useless
    would pass the value tests through the fallback alone."""
    n = 12000
    x = mo.gaussian_mixture(n, d, seed=d)
    monkeypatch.setenv("MELLON_AMD_NN_PREFILTER_MIN", "1")
    monkeypatch.setenv("MELLON_AMD_NN_PREFILTER", "1")
    ctx.nn_distances(x)
    last = ctx.nn_last()
    print(f"d={d}: {int(last[1])} of {n} rows open ({100.0 * last[1] / n:.2f} %)")
    assert last[0] == 4
    assert last[1] <= 0.25 * n


# ---- 4. k-means ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _km_cells(n, d, scaled):
    x = mo.gaussian_mixture(n, d, seed=d)
    return np.ascontiguousarray(x * 1e3 + 5e3) if scaled else x


@functools.lru_cache(maxsize=None)
def _sklearn_inertia(n, d, m, scaled):
    from sklearn.cluster import k_means
    return k_means(_km_cells(n, d, scaled), m, n_init=1, random_state=42)[2]


@pytest.mark.parametrize("n,d,m,scaled", [(60000, 65, 300, False), (60000, 128, 300, False), (40000, 256, 450, False),
                                          (60000, 128, 300, True)])
def test_wide_kmeans(ctx, monkeypatch, n, d, m, scaled):
    """The wide tier (n m >= 2^24): finite centres, the returned inertia is the centres' own, sklearn's quality, the same
    result from the same seed, the all-fp64 path's quality, nearly every centre owns a cell -- also in raw-count units with
    a large offset (scaled)."""
    from sklearn.metrics import pairwise_distances_argmin_min
    x = _km_cells(n, d, scaled)
    monkeypatch.setenv("MELLON_AMD_KM_FP16", "1")
    c, n_iter, inertia = ctx.kmeans(x, m, seed=42, return_info=True)
    assert c.shape == (m, d) and np.all(np.isfinite(c)) and 1 <= n_iter <= 600
    lab, dist = pairwise_distances_argmin_min(x, c)
    assert abs(np.sum(dist**2) - inertia) < 1e-6 * inertia
    assert inertia < 1.05 * _sklearn_inertia(n, d, m, scaled)
    c2 = ctx.kmeans(x, m, seed=42)
    assert np.abs(c2 - c).max() / np.abs(c).max() < 1e-9
    monkeypatch.setenv("MELLON_AMD_KM_FP16", "0")
    c0, it0, inertia0 = ctx.kmeans(x, m, seed=42, return_info=True)
    assert abs(inertia / inertia0 - 1) < 0.02
    assert len(np.unique(lab)) > 0.98 * m


def test_wide_kmeans_two_levels(ctx, monkeypatch):
    n, d, m = 200000, 65, 256
    x = mo.gaussian_mixture(n, d, seed=17)
    monkeypatch.setenv("MELLON_AMD_KM_FP16", "1")
    c1, it1, inertia1 = ctx.kmeans(x, m, seed=3, return_info=True)
    monkeypatch.setenv("MELLON_AMD_KM_FP16", "0")
    c0, it0, inertia0 = ctx.kmeans(x, m, seed=3, return_info=True)
    assert np.all(np.isfinite(c1)) and np.all(np.isfinite(c0))
    assert abs(inertia1 / inertia0 - 1) < 0.02


def test_wide_kmeans_edges(ctx):
    from mellon_amd import _lib
    small = mo.gaussian_mixture(50, 200, seed=2)
    cs = ctx.kmeans(small, 50, seed=1)
    assert np.allclose(np.sort(cs, axis=0), np.sort(small, axis=0))
    with pytest.raises(ValueError, match="256"):                    # (shape errors of the library are ValueErrors)
        ctx.kmeans(np.zeros((300, 257)), 3)
    with pytest.raises(ValueError, match="d <= 64"):
        ctx.kmeans(mo.gaussian_mixture(300, 65, seed=1), 3, init="sklearn")
    bad = mo.gaussian_mixture(1000, 100, seed=3)
    bad[17, 60] = np.nan
    with pytest.raises(_lib.MellonHipError, match="non-finite"):
        ctx.kmeans(bad, 10)


# ---- 5. through the public classes ------------------------------------------------------------------------------------------
def test_density_estimator_on_wide_cells(mellon, monkeypatch, caplog):
    """The default landmark and nearest-neighbour steps on 96 features, above the device threshold: the landmarks come from
    the device.  (d is passed: the estimator refuses a DETECTED dimensionality above 50, wherever its steps run.)"""
    from mellon_amd import parameters
    monkeypatch.setattr(parameters, "KMEANS_DEVICE_THRESHOLD", 1e6)
    n, d, m = 20000, 96, 200
    x = mo.gaussian_mixture(n, d, seed=96)
    est = mellon.DensityEstimator(n_landmarks=m, d=d)
    with caplog.at_level(logging.INFO, logger="mellon"):
        dens = est.fit_predict(x)
    assert any("backend=hip" in r.getMessage() for r in caplog.records)
    assert est.landmarks.shape == (m, d) and np.all(np.isfinite(est.landmarks))
    assert np.abs(est.nn_distances / mo.exact_nn_distances(x) - 1).max() < 1e-12
    assert np.all(np.isfinite(dens))
    assert np.abs(est.predict(x) - dens).max() / np.abs(dens).max() < 1e-9


def test_time_sensitive_estimator_on_wide_cells(mellon, monkeypatch, caplog):
    """64 state columns and the time column: d = 65 inside."""
    from mellon_amd import parameters
    monkeypatch.setattr(parameters, "KMEANS_DEVICE_THRESHOLD", 1e6)
    n, d, m = 20000, 64, 200
    x = mo.gaussian_mixture(n, d, seed=64)
    times = np.repeat([0.0, 1.0, 2.0], [7000, 7000, 6000]).astype(np.float64)
    est = mellon.TimeSensitiveDensityEstimator(n_landmarks=m, ls_time=1.0, d=d)
    with caplog.at_level(logging.INFO, logger="mellon"):
        dens = est.fit_predict(x, times)
    assert any("backend=hip" in r.getMessage() for r in caplog.records)
    assert est.landmarks.shape == (m, d + 1) and np.all(np.isfinite(est.landmarks))
    want = np.concatenate([mo.exact_nn_distances(x[times == t]) for t in (0.0, 1.0, 2.0)])
    assert np.abs(est.nn_distances / want - 1).max() < 1e-12
    assert np.all(np.isfinite(dens))
    assert np.abs(est.predict(x, times) - dens).max() / np.abs(dens).max() < 1e-9
