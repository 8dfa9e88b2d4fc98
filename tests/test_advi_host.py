"""ADVI on the host: the NumPy restatement the device tests compare against is itself checked here -- its gradients
against central finite differences of its own value, the draws, and the reference's own property (tests/test_laplace.py:
170-193 there): the ADVI mean's log-density correlates with the MAP log-density."""
import inspect

import numpy as np
import pytest

from oracle import mellon_oracle as mo
import advi_restatement as ar


@pytest.fixture(scope="module")
def blobs():
    X = ar.two_blobs(200, 2)
    fit = mo.density_fit(X, n_landmarks=20)
    V, Vdr = mo.nn_likelihood_constants(fit.nn_distances, fit.d)
    return fit, V, Vdr


def test_restatement_gradients_against_finite_differences(blobs):
    fit, V, Vdr = blobs
    L, mu = fit.L, fit.mu
    m = L.shape[1]
    rng = np.random.default_rng(3)
    mean = fit.initial_value + 0.1 * rng.standard_normal(m)
    log_std = -1.0 + 0.3 * rng.standard_normal(m)
    eps = ar.advi_draws(5, 7, m)
    _, gm, gs = ar.elbo_value_and_grad(mean, log_std, eps, L, mu, V, Vdr)
    h = 1e-5
    for j in range(m):
        e = np.zeros(m)
        e[j] = h
        fm = (ar.elbo_value_and_grad(mean + e, log_std, eps, L, mu, V, Vdr)[0]
              - ar.elbo_value_and_grad(mean - e, log_std, eps, L, mu, V, Vdr)[0]) / (2 * h)
        fs = (ar.elbo_value_and_grad(mean, log_std + e, eps, L, mu, V, Vdr)[0]
              - ar.elbo_value_and_grad(mean, log_std - e, eps, L, mu, V, Vdr)[0]) / (2 * h)
        # central differences: truncation h^2 f''' / 6 ~ 1e-10 relative, rounding eps |value| / h ~ 1e-8 absolute
        assert abs(fm - gm[j]) < 1e-6 * max(1.0, np.abs(gm).max()), (j, fm, gm[j])
        assert abs(fs - gs[j]) < 1e-6 * max(1.0, np.abs(gs).max()), (j, fs, gs[j])


def test_draws_are_deterministic_in_the_step():
    from mellon_amd import inference
    a, b = inference.advi_draws(3, 40, 17), inference.advi_draws(3, 40, 17)
    assert a.shape == (40, 17) and np.array_equal(a, b)
    assert not np.array_equal(a, inference.advi_draws(4, 40, 17))
    assert np.array_equal(a, ar.advi_draws(3, 40, 17))
    assert np.array_equal(a, np.random.default_rng(3).standard_normal((40, 17)))
    sig = inspect.signature(inference.run_advi)
    assert list(sig.parameters) == ["loss_func", "initial_parameters", "n_iter", "init_learn_rate", "nsamples", "jit"]
    assert sig.parameters["nsamples"].default == 40 == inference.DEFAULT_NUM_SAMPLES


def test_plain_callable_is_refused():
    from mellon_amd import inference
    with pytest.raises(NotImplementedError):
        inference.run_advi(lambda z: float(np.sum(z ** 2)), np.zeros(3))


def test_advi_mean_correlates_with_map_and_std_with_laplace(blobs):
    fit, V, Vdr = blobs
    L, mu = fit.L, fit.mu
    mean, std, losses = ar.run_advi(fit.initial_value, L, mu, V, Vdr, n_iter=200)
    assert losses.shape == (200,) and np.isfinite(losses).all() and np.all(std > 0)
    f_map, f_advi = L @ fit.pre_transformation + mu, L @ mean + mu
    corr = np.corrcoef(f_map, f_advi)[0, 1]
    lap = mo.laplace_std(fit.pre_transformation, L, mu, V)
    corr_std = np.corrcoef(std, lap)[0, 1]
    print(f"corr(MAP, ADVI) = {corr:.4f}, max |df| = {np.abs(f_map - f_advi).max():.3f}, corr(std, Laplace) = {corr_std:.4f}")
    assert corr > 0.8
    assert corr_std > 0.9
