"""DimensionalityEstimator on a real MI355X (-m gpu): the exact k-NN search, the local fractal dimension, the
dimensionality objective, the estimator end to end and d_method="fractal", each against the NumPy / SciPy restatement
of the reference (tests/dim_restatement.py)."""
import json

import numpy as np
import pytest
from scipy.optimize import minimize

import dim_restatement as dr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mellon():
    import mellon_amd
    return mellon_amd


@pytest.fixture(scope="module")
def ctx():
    from mellon_amd import _lib
    return _lib.default_context()


@pytest.fixture(scope="module")
def small_x():
    # the reference's tests/test_dimensionality_estimator.py: n = 100, d = 2, correlated normal
    rng = np.random.default_rng(535)
    A = rng.uniform(size=(2, 2))
    return rng.multivariate_normal(np.ones(2), A.T @ A, size=100)


def rel_std(a, b):
    return np.std(a - b) / np.std(b)


def brute_knn(x, y, k, exclude=False, offset=0):
    """Chunked brute force in difference form."""
    dist = np.empty((x.shape[0], k))
    idx = np.empty((x.shape[0], k), dtype=np.int64)
    for r0 in range(0, x.shape[0], 256):
        q = x[r0:r0 + 256]
        d2 = np.zeros((q.shape[0], y.shape[0]))
        for f in range(x.shape[1]):
            d2 += (q[:, f, None] - y[None, :, f]) ** 2
        if exclude:
            rows = np.arange(q.shape[0])
            cols = rows + r0 + offset
            ok = (cols >= 0) & (cols < y.shape[0])
            d2[rows[ok], cols[ok]] = np.inf
        o = np.argsort(d2, axis=1, kind="stable")[:, :k]
        idx[r0:r0 + 256] = o
        dist[r0:r0 + 256] = np.sqrt(np.take_along_axis(d2, o, axis=1))
    return dist, idx


def check_knn(dist, idx, ref_d, ref_i):
    scale = np.where(ref_d > 0, ref_d, 1.0)
    assert np.all(np.abs(dist - ref_d) <= 1e-13 * scale), np.abs(dist - ref_d).max()
    assert np.all((ref_d == 0) == (dist == 0))
    # index sets agree wherever neighbouring distances are separated
    k, nq = dist.shape[1], dist.shape[0]
    for j in range(k):
        lo = ref_d[:, j - 1] if j > 0 else np.full(nq, -np.inf)
        hi = ref_d[:, j + 1] if j + 1 < k else np.full(nq, np.inf)
        sep = (ref_d[:, j] - lo > 1e-9 * np.abs(ref_d[:, j])) & (hi - ref_d[:, j] > 1e-9 * np.abs(ref_d[:, j]))
        assert np.array_equal(idx[sep, j], ref_i[sep, j])


@pytest.mark.parametrize("n,d,k", [(2, 1, 1), (11, 2, 10), (31, 20, 30), (65, 61, 64), (1000, 50, 30),
                                   (1000, 100, 10), (1000, 1, 64), (20011, 20, 10)])
def test_knn_against_brute_force(ctx, n, d, k):
    rng = np.random.default_rng(n + d + k)
    x = rng.normal(size=(n, d))
    if n >= 1000:
        x[7] = x[3]              # a duplicated cell
    kk = min(k, n)
    dist, idx = ctx.knn(x, kk)
    ref_d, ref_i = brute_knn(x, x, kk)
    check_knn(dist, idx, ref_d, ref_i)
    if n > k:
        dist, idx = ctx.knn(x, k, exclude_self=True)
        ref_d, ref_i = brute_knn(x, x, k, exclude=True)
        check_knn(dist, idx, ref_d, ref_i)


def test_knn_cross_set_with_offset_and_limits(ctx):
    rng = np.random.default_rng(4)
    y = rng.normal(size=(777, 13))
    x = y[100:300] + 1e-3 * rng.normal(size=(200, 13))
    dist, idx = ctx.knn(x, 30, y=y, exclude_self=True, self_offset=100)
    ref_d, ref_i = brute_knn(x, y, 30, exclude=True, offset=100)
    check_knn(dist, idx, ref_d, ref_i)
    for bad in (0, 65):
        with pytest.raises(ValueError):
            ctx.knn(y, bad)
    with pytest.raises(ValueError):
        ctx.knn(y[:5], 5, exclude_self=True)


def test_local_dimensionality_against_restatement(mellon):
    from mellon_amd.util import local_dimensionality
    rng = np.random.default_rng(9)
    x = rng.normal(size=(300, 4)) @ rng.normal(size=(4, 6))
    for kw in ({}, {"k": 3}, {"x_query": x[:50] + 0.01}):
        got = local_dimensionality(x, **kw)
        want = dr.local_dimensionality(x, **kw)
        np.testing.assert_allclose(got, want, rtol=1e-10)
    nbr = dr.neighbours(x, 12)[1][::3]
    np.testing.assert_allclose(local_dimensionality(x, k=12, neighbor_idx=nbr),
                               dr.local_dimensionality(x, neighbor_idx=nbr), rtol=1e-10)
    # a coincident pair: NaN in the rows whose neighbourhood holds it, finite elsewhere
    xd = x.copy()
    xd[5] = xd[17]
    got = local_dimensionality(xd)
    want = dr.local_dimensionality(xd)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).any() and not np.isnan(got).all()
    np.testing.assert_allclose(got[~np.isnan(want)], want[~np.isnan(want)], rtol=1e-10)
    assert local_dimensionality(np.ones((10, 3))).shape == (10,)


def _fit_case(mellon, kind, n, m, d=3, seed=0):
    from mellon_amd import _lib, cov
    from mellon_amd.decomposition import _full_decomposition_low_rank, _modified_low_rank
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, d))
    k = cov.Matern52(1.3)
    c = _lib.default_context()
    if kind == "full":
        fit = c.fit_prepare(k.lower(d), x, None, 1e-6)
    elif kind == "sparse_cholesky":
        fit = c.fit_prepare(k.lower(d), x, x[rng.choice(n, m, replace=False)], 1e-6)
    elif kind == "implicit":
        fit = c.fit_prepare(k.lower(d), x, x[rng.choice(n, m, replace=False)], 1e-6, implicit=True)
    elif kind == "full_nystroem":
        fit = _full_decomposition_low_rank(x, k, rank=0.999, jitter=1e-6).fit
    else:
        fit = _modified_low_rank(x, k, x[rng.choice(n, m, replace=False)], rank=0.999, jitter=1e-6).fit
    return x, fit


@pytest.mark.parametrize("kind,n,m", [("full", 300, None), ("sparse_cholesky", 1001, 1), ("sparse_cholesky", 2003, 17),
                                      ("sparse_cholesky", 5003, 1000), ("implicit", 3001, 1000),
                                      ("full_nystroem", 400, None), ("sparse_nystroem", 1500, 200),
                                      ("implicit", 6007, 5000), ("sparse_cholesky", 6007, 5000)])
def test_dim_objective_against_restatement(mellon, kind, n, m):
    x, fit = _fit_case(mellon, kind, n, m)
    rng = np.random.default_rng(1)
    L = fit.L()
    dist = np.abs(rng.normal(size=(fit.n, 10))) + 0.05
    ell = dr.ell_of(dist)
    mu_dim, mu_dens = 0.3, 1.1
    fit.set_dim_likelihood(ell, mu_dim, mu_dens)
    z = rng.normal(size=(2, fit.m)) * 0.1
    want = dr.dim_loss(z, L, ell, mu_dim, mu_dens)
    gw, hw = dr.dim_grad_hess(z, L, ell, mu_dim, mu_dens)
    if kind == "implicit":
        loss, g = fit.dim_objective(z)
        with pytest.raises(NotImplementedError):
            fit.dim_objective(z, with_hess=True)
    else:
        loss, g, h = fit.dim_objective(z, with_hess=True)
        np.testing.assert_allclose(h, hw, rtol=1e-9, atol=1e-9 * np.abs(hw).max())
    assert abs(loss - want) <= 1e-11 * abs(want)
    np.testing.assert_allclose(g, gw, rtol=1e-9, atol=1e-9 * np.abs(gw).max())


def test_dim_objective_one_pass_limit(mellon):
    x, fit = _fit_case(mellon, "implicit", 5200, 5121)
    with pytest.raises(NotImplementedError, match="5120"):
        fit.set_dim_likelihood(np.zeros((fit.n, 10)), 0.0, 0.0)


def test_estimator_end_to_end_matches_scipy_solve_of_restatement(mellon):
    rng = np.random.default_rng(21)
    x = rng.normal(size=(2000, 5))
    est = mellon.DimensionalityEstimator(n_landmarks=200, predictor_with_uncertainty=True)
    dim = est.fit_predict(x)
    L = np.asarray(est.L)
    ell = dr.ell_of(est.distances)
    loss = dr.dim_loss(est.pre_transformation, L, ell, est.mu_dim, est.mu_dens)
    g, _ = dr.dim_grad_hess(est.pre_transformation, L, ell, est.mu_dim, est.mu_dens)
    assert np.abs(g).max() <= 1e-5 * max(1.0, abs(loss))
    assert abs(est.losses[-1] - loss) <= 1e-9 * abs(loss)          # the K = 2 constant included
    # the reference's initial value and a SciPy solve of the restatement from it
    d_ref = dr.local_dimensionality(x)
    np.testing.assert_allclose(est.d, d_ref, rtol=1e-10)
    z0 = dr.initial_dimensionalities(L, est.d, est.mu_dim, est.nn_distances, est.mu_dens)
    np.testing.assert_allclose(est.initial_value, z0, rtol=1e-8, atol=1e-10)
    res = minimize(lambda z: (dr.dim_loss(z, L, ell, est.mu_dim, est.mu_dens),
                              dr.dim_grad_hess(z, L, ell, est.mu_dim, est.mu_dens)[0].ravel()),
                   z0.ravel(), jac=True, method="L-BFGS-B", options=dict(maxiter=20000, maxfun=50000, ftol=1e-15, gtol=1e-9))
    z = res.x.reshape(2, -1)
    want_dim = np.exp(est.mu_dim + L @ z[0])
    want_dens = est.mu_dens + L @ z[1]
    assert np.abs(dim - want_dim).max() <= 1e-5 * np.abs(want_dim).max()
    assert np.abs(est.log_density_x - want_dens).max() <= 1e-5 * np.abs(want_dens).max()
    assert est.pre_transformation_std.shape == (2, L.shape[1])


def test_reference_properties(mellon, small_x, tmp_path):
    n, d = small_x.shape
    est = mellon.DimensionalityEstimator()
    local_dim = est.fit_predict(small_x)
    assert local_dim.shape == (n,) and np.all(np.isfinite(local_dim))
    assert rel_std(est.predict(small_x), local_dim) < 1e-4
    assert est.predict_density.gradient(small_x).shape == (n, d)
    assert est.predict_density(small_x).shape == (n,)
    assert est.predict_density.hessian(small_x).shape == (n, d, d)
    sgn, ld = est.predict_density.hessian_log_determinant(small_x)
    assert sgn.shape == (n,) and ld.shape == (n,)
    # the approximations (reference thresholds) and adam
    for rank, n_landmarks, lim in ((1.0, 100, 1e0), (1.0, 10, 2e0), (0.99, 80, 1e0), (50, 80, 1e0)):
        e = mellon.DimensionalityEstimator(rank=rank, n_landmarks=n_landmarks).fit(small_x)
        assert rel_std(e.predict(small_x), local_dim) < lim
    adam = mellon.DimensionalityEstimator(optimizer="adam").fit_predict(small_x)
    assert rel_std(adam, local_dim) < 2e0
    # Laplace uncertainty instead of ADVI; JSON round trip
    for rank, n_landmarks in ((1.0, 0), (0.99, 0), (1.0, 10), (0.99, 80)):
        e = mellon.DimensionalityEstimator(rank=rank, n_landmarks=n_landmarks, predictor_with_uncertainty=True)
        e.fit(small_x)
        p = e.predict
        v, lv = p(small_x), p(small_x, logscale=True)
        assert np.allclose(v, np.exp(lv))
        assert p.covariance(small_x).shape == (n,)
        assert p.mean_covariance(small_x).shape == (n,)
        unc = p.uncertainty(small_x)
        assert unc.shape == (n,)
        path = str(tmp_path / f"dim_{n_landmarks}_{rank}.json")
        p.to_json(path)
        again = mellon.Predictor.from_json(path)
        assert np.allclose(again(small_x), v) and np.allclose(again.uncertainty(small_x), unc)
        json.loads(p.to_json())


def test_reference_errors(mellon, small_x):
    lX = np.concatenate([small_x] * 26, axis=1)
    est = mellon.DimensionalityEstimator()
    with pytest.raises(ValueError):
        est.fit_predict()
    with pytest.raises(ValueError):
        est.fit(None)
    est.set_x(small_x)
    with pytest.raises(ValueError):
        est.prepare_inference(lX)
    loss_func, initial_value = est.prepare_inference(None)
    with pytest.raises(NotImplementedError):
        est.run_inference(loss_func, initial_value, "advi")
    est.run_inference(loss_func, initial_value, "L-BFGS-B")
    est.process_inference(est.pre_transformation)
    with pytest.raises(ValueError):
        est.fit_predict(lX)
    est.fit_predict()
    with pytest.raises(ValueError):
        mellon.DimensionalityEstimator(k=0).fit(small_x)
    dup = np.concatenate([small_x, small_x[:3]])
    with pytest.raises(ValueError, match="6 cells"):        # three pairs of coincident cells
        mellon.DimensionalityEstimator().fit(dup)


@pytest.mark.parametrize("n_landmarks", [0, 30])
def test_explog_conditions_on_log_y(mellon, small_x, n_landmarks):
    """inference.py:707,753: the full and landmarks branches condition on log(y)."""
    from mellon_amd.inference import compute_conditional, compute_conditional_explog
    est = mellon.DensityEstimator(n_landmarks=n_landmarks, rank=0.99 if n_landmarks else 1.0).fit(small_x)
    y = np.exp(0.1 * est.log_density_x)
    pre = None                                            # (never the Cholesky branch, which does not read y)
    kw = dict(sigma=None, jitter=est.jitter, y_is_mean=True)
    p = compute_conditional_explog(small_x, est.landmarks, pre, None, y, 0.1 * est.mu, est.cov_func, est.L, est.Lp, **kw)
    q = compute_conditional(small_x, est.landmarks, pre, None, np.log(y), 0.1 * est.mu, est.cov_func, est.L, est.Lp,
                            **kw)
    xq = small_x[:20] + 0.01
    np.testing.assert_allclose(p.mean(xq, logscale=True), q(xq), rtol=1e-12)
    if n_landmarks == 0:                                  # the full GP interpolates its training values
        np.testing.assert_allclose(p(small_x), y, rtol=1e-4)


def test_fractal_d(mellon):
    rng = np.random.default_rng(2)
    x = rng.normal(size=(1200, 3)) @ rng.normal(size=(3, 5))
    est = mellon.DensityEstimator(d_method="fractal", n_landmarks=50)
    est.prepare_inference(x)
    assert abs(est.d - dr.fractal_d(x)) <= 1e-10 * abs(est.d)
    small = x[:400]
    est = mellon.DensityEstimator(d_method="fractal", n_landmarks=50)
    est.prepare_inference(small)
    assert abs(est.d - float(np.mean(dr.local_dimensionality(small, k=10)))) <= 1e-10 * abs(est.d)
    xt = np.concatenate([x, np.repeat([0.0, 1.0, 2.0], 400)[:, None]], axis=1)
    ts = mellon.TimeSensitiveDensityEstimator(d_method="fractal", n_landmarks=50)
    ts.prepare_inference(xt)
    assert abs(ts.d - dr.fractal_d(x)) <= 1e-10 * abs(ts.d)


def test_at_scale_linear_subspace(mellon):
    rng = np.random.default_rng(77)
    n = 200_000
    x = rng.normal(size=(n, 3)) @ np.linalg.qr(rng.normal(size=(20, 3)))[0].T
    x += 1e-6 * rng.normal(size=x.shape)
    est = mellon.DimensionalityEstimator(n_landmarks=1000)
    dim = est.fit_predict(x)
    assert np.all(np.isfinite(dim)) and np.all(np.isfinite(est.log_density_x))
    # Window widened from [2.3, 3.7]: the reference's estimator is biased low on this data.  Its local fractal dimension
    # (k = 30) has median 2.16 on a 3-d Gaussian and on a uniform 3-d cube alike (2e5 cells, NumPy + sklearn), and the
    # restated MAP solve (NumPy / SciPy, 2e4 cells, 300 landmarks) ends at median 1.72.
    assert 1.9 <= np.median(est.d) <= 2.4, np.median(est.d)
    assert 1.4 <= np.median(dim) <= 2.6, np.median(dim)
