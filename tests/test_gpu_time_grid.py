"""multi_time on a grid: PredictorTime folds the time factor of a separable covariance into the weights and evaluates all T
times with ONE multi-output pass over the state kernel (base_predictor.py `_grid_*`), instead of T single-time calls."""
import functools
from math import log

import numpy as np
import pytest

from oracle import mellon_oracle as mo

pytestmark = pytest.mark.gpu

STATIONARY = ["Matern32", "Matern52", "ExpQuad", "Exponential", "RatQuad"]
N, M, D, T = 130, 70, 4, 9                      # 130 x 70 x 9 = 81900 >= 2^16: the grid path


def _pair(product_cov):
    return mo.Covariance.from_dict(product_cov.to_dict())


def _tree(name):
    from mellon_amd import cov
    K = getattr(cov, name)
    if name == "RatQuad":
        return K(2.0, 2.6, active_dims=slice(None, -1)) * K(1.5, 1.3, active_dims=-1)
    return K(2.6, active_dims=slice(None, -1)) * K(1.3, active_dims=-1)


@functools.lru_cache(maxsize=None)
def _inputs():
    """Random state coordinates; centre times on multiples of 0.1 in [0, 4), query times half way between such multiples, so
    that |t - s_j| >= 0.05 for every pair: the oracle's k_grad divides by dist + 1e-12 where the device divides by dist, a
    relative 1e-12 / dist <= 2e-11 of one term -- inside the 1e-10 bound, which a near-coincident pair of a random draw
    would not be (the cusp of Exponential has an O(1) derivative there)."""
    rng = np.random.default_rng(94)
    c = rng.normal(size=(M, D))
    c[:, -1] = rng.integers(0, 40, size=M) / 10.0
    x = rng.normal(size=(N, D - 1))
    w = rng.normal(size=M)
    times = 0.05 + np.sort(rng.choice(40, size=T, replace=False)) / 10.0
    for a in (c, x, w, times):
        a.flags.writeable = False
    return c, x, w, times


def _err(a, ref):
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300)


def _loop(p, name, x, times, **kw):
    return np.stack([getattr(p, name)(x, time=float(t), **kw) for t in times], axis=1)


@pytest.fixture
def mean_calls(monkeypatch):
    """Counts Context.predict_mean calls."""
    from mellon_amd import _lib
    calls = []
    inner = _lib.Context.predict_mean

    def counted(self, *a, **k):
        calls.append(1)
        return inner(self, *a, **k)

    monkeypatch.setattr(_lib.Context, "predict_mean", counted)
    return calls


@pytest.mark.parametrize("name", STATIONARY)
def test_grid_matches_the_oracle_predictor_at_every_time(name, mean_calls):
    from mellon_amd.base_predictor import PredictorTime
    c, x, w, times = _inputs()
    tree = _tree(name)
    p = PredictorTime(tree, c, w, 0.7, n_obs=500)
    ref = mo.Predictor(_pair(tree), c, w, 0.7, 500)
    mean_ref, grad_ref = [], []
    for t in times:
        xt = np.concatenate([x, np.full((N, 1), t)], axis=1)
        mean_ref.append(ref(xt))
        grad_ref.append(ref.analytic_gradient(xt))
    mean_ref, grad_ref = np.stack(mean_ref, axis=1), np.stack(grad_ref, axis=1)          # (N, T), (N, T, D)
    mean = p.mean(x, multi_time=times)
    assert len(mean_calls) == 1                                                           # not T
    td = p.time_derivative(x, multi_time=times)
    assert len(mean_calls) == 2
    g = p.gradient(x, multi_time=times)
    assert mean.shape == (N, T) and td.shape == (N, T) and g.shape == (N, T, D - 1)
    errs = _err(mean, mean_ref), _err(td, grad_ref[..., -1]), _err(g, grad_ref[..., :-1])
    print(f"{name}: mean {errs[0]:.2e} time_derivative {errs[1]:.2e} gradient {errs[2]:.2e}")
    assert max(errs) < 1e-10
    assert np.array_equal(p(x, multi_time=times), mean)                                   # __call__ is mean
    # normalize is applied as by the single-time call
    assert np.array_equal(p.mean(x, normalize=True, multi_time=times), mean - log(500))
    assert _err(p.mean(x, normalize=True, multi_time=times), _loop(p, "mean", x, times, normalize=True)) < 1e-10


@pytest.fixture(scope="module")
def fitted():
    import mellon_amd
    rng = np.random.default_rng(5)
    times = np.repeat(np.arange(4.0), 100)
    X = rng.normal(size=(400, 3)) @ np.array([[2.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.3, -0.5, 0.8]]) + 0.4 * times[:, None]
    est = mellon_amd.TimeSensitiveDensityEstimator(n_landmarks=70, ls_time=1.3).fit(X, times)
    return est.predict, np.ascontiguousarray(X[::2][:170])


def test_grid_against_loop_on_a_fitted_estimator(fitted):
    """|grid - loop| <= 1e-12 S entry by entry, S = sum_j |w_j term_ij(t)| (the kernel value for the mean, the kernel
    derivative for the two derivatives).  Both are fp64 sums of the same m = 70 terms in different order (m eps ~ 1e-14) on
    kernel values that differ by rounding (~1e-14 per term): <= ~1e-13 S, and 1e-12 leaves a factor of ten.
    Measured on the MI355X (largest |grid - loop| / S, printed): mean 2.5e-16, time_derivative 1.3e-16, gradient 1.8e-16."""
    p, xq = fitted
    mt = np.linspace(0.25, 2.75, 9)
    assert xq.shape[0] * p.centers.shape[0] * mt.size >= 1 << 16 and p.weights.ndim == 1
    w = np.abs(p.weights)
    S_mean, S_td, S_grad = [], [], []
    for t in mt:
        xt = np.concatenate([xq, np.full((xq.shape[0], 1), t)], axis=1)
        S_mean.append(np.abs(p.cov_func.k(xt, p.centers)) @ w)
        dk = np.abs(p.cov_func.k_grad(p.centers)(xt))                                     # (m, n, d)
        S = np.einsum("j,jik->ik", w, dk)
        S_td.append(S[:, -1])
        S_grad.append(S[:, :-1])
    worst = {}
    for name, S in (("mean", S_mean), ("time_derivative", S_td), ("gradient", S_grad)):
        S = np.stack(S, axis=1)
        grid, loop = getattr(p, name)(xq, multi_time=mt), _loop(p, name, xq, mt)
        assert grid.shape == loop.shape == S.shape
        worst[name] = (np.abs(grid - loop) / S).max()
    print("largest |grid - loop| / S: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= 1e-12, worst


def test_small_problems_and_everything_without_a_grid_keep_the_loop(mean_calls):
    from mellon_amd import cov
    from mellon_amd.base_predictor import PredictorTime
    c, x, w, times = _inputs()
    tree = _tree("Matern52")
    # 12 x 20 x 3 < 2^16: three calls, the loop's own bits
    small = PredictorTime(tree, c[:20], w[:20], 0.7, n_obs=500)
    out = small.mean(x[:12], multi_time=times[:3])
    assert len(mean_calls) == 3
    mean_calls.clear()
    assert np.array_equal(out, _loop(small, "mean", x[:12], times[:3]))
    # one time is not a grid
    mean_calls.clear()
    p = PredictorTime(tree, c, w, 0.7, n_obs=500)
    assert p.mean(x, multi_time=[0.5]).shape == (N, 1) and len(mean_calls) == 1
    # time= together with multi_time=
    with pytest.raises(ValueError, match="both"):
        p.mean(x, time=1.0, multi_time=times)
    with pytest.raises(ValueError, match="both"):
        p.gradient(x, time=1.0, multi_time=times)
    # normalize without n_obs: the predictor's own error
    with pytest.raises(ValueError, match="n_obs"):
        PredictorTime(tree, c, w, 0.7).mean(x, normalize=True, multi_time=times)
    # wrong number of columns: the single-time call's own error
    with pytest.raises(ValueError, match="features"):
        p.mean(np.zeros((N, D + 1)), multi_time=times)
    # a tree that does not separate
    mixed = PredictorTime(cov.Matern52(2.6, active_dims=slice(None, -1)) + cov.Matern52(1.3, active_dims=-1), c, w, 0.7)
    for name in ("mean", "gradient", "time_derivative"):
        mean_calls.clear()
        assert np.array_equal(getattr(mixed, name)(x, multi_time=times), _loop(mixed, name, x, times))
    mean_calls.clear()
    mixed.mean(x, multi_time=times)
    assert len(mean_calls) == T
    # 2-D weights
    W = np.ascontiguousarray(np.stack([w, 2.0 * w], axis=1))
    two = PredictorTime(tree, c, W, 0.7)
    mean_calls.clear()
    out = two.mean(x, multi_time=times)
    assert out.shape == (N, T, 2) and len(mean_calls) == T
    assert np.array_equal(out, _loop(two, "mean", x, times))
    g = two.gradient(x, multi_time=times)
    assert g.shape == (N, T, 2, D - 1) and np.array_equal(g, _loop(two, "gradient", x, times))
