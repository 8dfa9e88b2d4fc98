"""DimensionalityEstimator on the host (no GPU): the public surface and the restatement the GPU tests check against."""
import numpy as np
import pytest

import dim_restatement as dr


def test_estimator_exists_with_reference_defaults():
    import mellon_amd
    est = mellon_amd.DimensionalityEstimator()
    # reference dimensionality_estimator.py:177-241
    assert est.k == 10 and est.mu_dim == 0 and est.mu_dens is None and est.distances is None
    assert est.optimizer == "L-BFGS-B" and est.jitter == 1e-6 and est.n_iter == 100
    assert est.local_dim_x is None and est.log_density_x is None
    assert est.local_dim_func is None and est.log_density_func is None
    assert "DimensionalityEstimator" in repr(est)
    from mellon_amd import inference, parameters, util
    for mod, name in ((parameters, "compute_d_factal"), (parameters, "compute_initial_dimensionalities"),
                      (util, "local_dimensionality"), (inference, "compute_dimensionality_transform"),
                      (inference, "compute_dimensionality_loss_func")):
        assert callable(getattr(mod, name))


def test_estimator_validation_errors():
    import mellon_amd
    with pytest.raises(ValueError):
        mellon_amd.DimensionalityEstimator(k=-1)
    with pytest.raises(ValueError):
        mellon_amd.DimensionalityEstimator(k=2.5)
    with pytest.raises(ValueError):
        mellon_amd.DimensionalityEstimator(optimizer="sgd")
    with pytest.raises(ValueError):
        mellon_amd.DimensionalityEstimator(mu_dim="a")
    est = mellon_amd.DimensionalityEstimator()
    with pytest.raises(ValueError):
        est.fit_predict()
    with pytest.raises(ValueError):
        est.fit(None)


def _case(seed=3, n=40, m=7, k=10):
    rng = np.random.default_rng(seed)
    L = rng.normal(size=(n, m)) * 0.3
    ell = dr.ell_of(rng.uniform(0.05, 2.0, size=(n, k)))
    z = rng.normal(size=(2, m)) * 0.2
    return L, ell, z


def test_restatement_gradient_and_hessian_agree_with_differences():
    L, ell, z = _case()
    mu_dim, mu_dens = 0.4, -1.3
    g, h = dr.dim_grad_hess(z, L, ell, mu_dim, mu_dens)
    step = 1e-5
    for r in range(2):
        for j in range(z.shape[1]):
            e = np.zeros_like(z)
            e[r, j] = step
            fp, fm = dr.dim_loss(z + e, L, ell, mu_dim, mu_dens), dr.dim_loss(z - e, L, ell, mu_dim, mu_dens)
            np.testing.assert_allclose(g[r, j], (fp - fm) / (2 * step), rtol=1e-6, atol=1e-7)
            gp = dr.dim_grad_hess(z + e, L, ell, mu_dim, mu_dens)[0][r, j]
            gm = dr.dim_grad_hess(z - e, L, ell, mu_dim, mu_dens)[0][r, j]
            np.testing.assert_allclose(h[r, j], (gp - gm) / (2 * step), rtol=1e-6, atol=1e-7)


def test_loss_carries_two_latent_functions_in_the_prior_constant():
    L, ell, z = _case(seed=5)
    assert abs(dr.dim_loss(z, L, ell, 0.0, 0.0) - dr.dim_loss(z, L, ell, 0.0, 0.0, K=4) + np.log(2 * np.pi)) < 1e-9


def test_closed_form_slope_equals_lstsq():
    rng = np.random.default_rng(11)
    for k in (3, 10, 30, 64):
        for d in (1, 2, 7, 50):
            nb = rng.normal(size=(k, d)) * rng.uniform(0.1, 3)
            nd = dr.pair_distances(nb)
            a, b = dr.slope_closed(nd), dr.slope_lstsq(nd)
            assert abs(a - b) <= 1e-12 * max(1.0, abs(b)), (k, d, a, b)


def _slope_cases():
    rng = np.random.default_rng(12)
    for k in (2, 3, 10, 30, 64):
        for d in (1, 2, 7, 50):
            yield f"gauss k={k} d={d}", dr.pair_distances(rng.normal(size=(k, d)) * rng.uniform(0.1, 3))
    for k in (3, 4, 10, 30, 64):
        yield f"one-hot k={k}", dr.pair_distances(dr.one_hot_rows(k))
        for s in range(3):
            yield f"simplex k={k} seed={s}", dr.pair_distances(dr.rotated_simplex(k, s))
            yield f"scaled simplex k={k} seed={s}", dr.pair_distances(dr.rotated_simplex(k, s) * 10.0 ** (s - 1))


def test_rank_rule_slope_equals_lstsq():
    """The device's rule (full rank: closed form; rank 1: minimum norm) is lstsq's, equidistant neighbourhoods included."""
    for name, nd in _slope_cases():
        a, b = dr.slope_rank_rule(nd), dr.slope_lstsq(nd)
        assert np.isfinite(a) and abs(a - b) <= 1e-10 * max(1.0, abs(b)), (name, a, b)


def test_equidistant_neighbourhoods_are_rank_deficient_for_lstsq():
    """The closed form alone is not lstsq's answer on an equidistant neighbourhood (0 / 0 or rounding noise), and the
    exact answer there is c ybar / (1 + c^2), c = log of the common distance."""
    for k in (3, 4, 10, 30, 64):
        kc2 = k * (k - 1) // 2
        c = np.log(np.sqrt(2.0))
        want = c * np.mean(np.log(np.arange(1, kc2 + 1))) / (1 + c * c)
        for nb in (dr.one_hot_rows(k), dr.rotated_simplex(k, k)):
            nd = dr.pair_distances(nb)
            assert abs(dr.slope_lstsq(nd) - want) <= 1e-12 * abs(want)
            with np.errstate(divide="ignore", invalid="ignore"):
                closed = dr.slope_closed(nd)
            assert not abs(closed - want) <= 1e-3 * abs(want), (k, closed, want)


def test_zero_distance_gives_nan():
    nd = dr.pair_distances(np.array([[0.0, 1.0], [0.0, 1.0], [2.0, 0.5]]))
    with np.errstate(divide="ignore", invalid="ignore"):
        assert np.isnan(dr.slope_rank_rule(nd)) and np.isnan(dr.slope_lstsq(nd))


def test_estimator_rejects_k_beyond_the_search_limit_before_device_work(monkeypatch):
    import mellon_amd
    from mellon_amd import _lib

    def no_device(*a, **kw):
        raise AssertionError("device work before the k check")
    monkeypatch.setattr(_lib, "default_context", no_device)
    x = np.random.default_rng(0).normal(size=(100, 3))
    with pytest.raises(ValueError, match="1 <= k <= 64"):
        mellon_amd.DimensionalityEstimator(k=65).prepare_inference(x)
    with pytest.raises(ValueError, match="1 <= k <= 64"):
        mellon_amd.DimensionalityEstimator(k=90).fit(x)
