"""covariance / mean_covariance / uncertainty with multi_time= on a grid: one mln_predict_variance_grid call for all T times
(base_predictor.py `_grid_variances`, csrc/predict_variance.hip) against the longdouble restatement of
variance_restatement.py, and the per-time loop wherever the grid does not apply.

Error measure, entry by entry: e(a) = max |a - restatement| / S with S = k** + sum A^2 for the covariance, sum (K W)^2 for
the mean covariance and their sum for the uncertainty.  The per-time loop of the same objects is measured in the same run and
the grid has to satisfy  e_grid <= 4 max(e_loop, m eps):  m eps bounds an m-term fp64 sum, the factor 4 is head-room for
the different summation order and the GEMM tile shapes on the tall panel.

The restatement of a predictor whose W came from _attach_uncertainty is the definition sum std^2 (L^-1 k)^2 with the exact
std; the loop reads the float64 W = L^-T diag(std) that a device solve rounded, and that rounding is part of e_loop.

Measured on the MI355X (printed with -s; largest over m = 130 / 128 and the four routes; the tiny budget gave the default's
figures): covariance e_grid 2.97e-15 (e_loop 2.97e-15), mean covariance 1.13e-14 (7.98e-15), uncertainty 2.93e-15
(2.93e-15), bound 1.1e-13.  Fitted estimator, L-BFGS-B / advi: covariance 4.87e-15 / 4.87e-15 (e_loop 4.81e-15 / 4.81e-15),
mean covariance 1.67e-13 / 1.08e-13 (2.08e-13 / 8.39e-14), uncertainty 1.16e-15 / 1.26e-15 (2.93e-15 / 3.17e-15); general W
after a JSON round trip against the std route: 0 / 1.57e-13 / 3.37e-15 of S at most."""
import functools

import numpy as np
import pytest

import variance_restatement as vr

pytestmark = pytest.mark.gpu

N, T = 131, 5
TIMES = np.linspace(0.25, 2.75, T)
EPS = np.finfo(np.float64).eps
METHODS = ("covariance", "mean_covariance", "uncertainty")
ROUTES = ("std", "general", "dense7", "cs")


def _tree():
    from mellon_amd import cov
    return cov.Matern52(vr.LS_STATE, active_dims=slice(None, -1)) * cov.Matern52(vr.LS_TIME, active_dims=-1)


def _pad16(v):
    return (v + 15) // 16 * 16


def chunking(n, n_times, m, q, budget):
    """(r, T_b) of mln_predict_variance_grid (csrc/predict_variance.hip): q = 0 unless a general W is passed."""
    ld, ldq = _pad16(m), (_pad16(q) if q else 0)
    budget = budget or 1 << 27
    r = max(64, min(budget // (2 * ld + ldq) // 64 * 64, min(32768, (n + 63) // 64 * 64)))
    return r, max(1, min((budget - r * ld) // (r * (ld + ldq)), n_times))


def tiny_budget(m, q):
    """The budget at which 131 queries go in chunks of 64, 64, 3 and 5 times in blocks of 2, 2, 1."""
    ld, ldq = _pad16(m), (_pad16(q) if q else 0)
    budget = 64 * (3 * ld + 2 * ldq)
    assert chunking(N, T, m, q, budget) == (64, 2)
    return budget


@functools.lru_cache(maxsize=None)
def _problem(m):
    c, x, L, std = vr.make_problem(N, m, seed=2024 + m)
    assert N * m * T >= 1 << 16                                   # the grid route, not the loop
    assert np.unique(x, axis=0).shape[0] == N                     # every query row distinct
    K, kxx = vr.product_kernel(x, TIMES, c)
    rng = np.random.default_rng(m)
    W7 = rng.normal(size=(m, 7)) * 0.2
    B = rng.normal(size=(m, 4)) * 0.3
    Cs = L @ np.linalg.cholesky(np.eye(m) + B @ B.T)
    for a in (W7, Cs):
        a.flags.writeable = False
    return c, x, L, std, K, kxx, W7, Cs


@functools.lru_cache(maxsize=None)
def _predictor(m, route):
    """(predictor, restatement dict, q of a general W or 0) for one route; the predictor is built by hand."""
    from mellon_amd.base_predictor import PredictorTime
    from mellon_amd.conditional import _attach_uncertainty
    c, x, L, std, K, kxx, W7, Cs = _problem(m)
    p = PredictorTime(_tree(), c, np.linspace(-1.0, 1.0, m), 0.3)
    if route == "std":
        _attach_uncertainty(p, L, std)
        assert p._grid_std() is not None and "_uncertainty_std" not in p._state_variables
        ref, q = vr.variances(K, kxx, L=L, std=std), 0
    elif route == "general":
        _attach_uncertainty(p, L, std)
        p.W = np.array(p.W)                                       # the same numbers as a plain array: the general route
        assert p._grid_std() is None
        ref, q = vr.variances(K, kxx, L=L, W=p.W), m
    elif route == "dense7":
        p.L, p.W = np.array(L), np.array(W7)
        ref, q = vr.variances(K, kxx, L=L, W=W7), 7
    else:
        p.L, p.W, p.Cs = np.array(L), np.array(W7), np.array(Cs)
        ref, q = vr.variances(K, kxx, L=L, Cs=Cs, W=W7), 7
    ref = {k: v.reshape(N, T) for k, v in ref.items()}
    return p, ref, q


def _ref_and_scale(ref, method):
    if method == "covariance":
        return ref["cov"], ref["S_cov"]
    if method == "mean_covariance":
        return ref["mcov"], ref["S_mcov"]
    return ref["cov"] + ref["mcov"], ref["S_cov"] + ref["S_mcov"]


def _e(a, ref, S):
    return float((np.abs(a.astype(np.longdouble) - ref) / S).max())


def _loop(p, method, x, times, **kw):
    return np.stack([getattr(p, method)(x, time=float(t), **kw) for t in times], axis=1)


seen_budgets = []          # the scratch_doubles keyword of every counted call, in order


@pytest.fixture
def calls(monkeypatch):
    """Counts the Context calls behind the variances, by name."""
    del seen_budgets[:]
    from mellon_amd import _lib
    seen = {"predict_covariance": 0, "predict_mean_covariance": 0, "predict_variance_grid": 0}
    budgets = seen_budgets

    def counted(name):
        inner = getattr(_lib.Context, name)

        def f(self, *a, **k):
            seen[name] += 1
            budgets.append(k.get("scratch_doubles"))
            return inner(self, *a, **k)
        return f

    for name in seen:
        monkeypatch.setattr(_lib.Context, name, counted(name))
    return seen


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("m", [130, 128])
def test_grid_against_the_restatement(m, route):
    """Every route at the default budget and at one so small that the queries go in chunks of 64, 64, 3 and the times in
    blocks of 2, 2, 1: both within the criterion, the tiny budget bit for bit the same when called twice."""
    p, ref, q = _predictor(m, route)
    x = _problem(m)[1]
    q_mcov = 0 if route == "std" else q
    for method in METHODS:
        r, S = _ref_and_scale(ref, method)
        e_loop = _e(_loop(p, method, x, TIMES), r, S)
        bound = 4 * max(e_loop, m * EPS)
        p._GRID_VARIANCE_DOUBLES = 0
        grid = getattr(p, method)(x, multi_time=TIMES)
        p._GRID_VARIANCE_DOUBLES = tiny_budget(m, 0 if method == "covariance" else q_mcov)
        try:
            tiny = getattr(p, method)(x, multi_time=TIMES)
            again = getattr(p, method)(x, multi_time=TIMES)
        finally:
            p._GRID_VARIANCE_DOUBLES = 0
        assert grid.shape == tiny.shape == (N, T)
        e_grid, e_tiny = _e(grid, r, S), _e(tiny, r, S)
        print(f"m={m} {route:8s} {method:16s} e_grid {e_grid:.2e} e_tiny {e_tiny:.2e} e_loop {e_loop:.2e} "
              f"bound {bound:.2e}")
        assert e_grid <= bound and e_tiny <= bound, (method, e_grid, e_tiny, e_loop)
        assert np.array_equal(tiny, again)


def test_shape_and_layout():
    """(n, T), column t = time t of np.stack(..., axis=1): every query row is distinct, and a swapped axis or a shifted
    chunk would put another row's or time's value -- which differs by far more than the tolerance -- in its place."""
    m = 130
    p, ref, _ = _predictor(m, "std")
    x = _problem(m)[1]
    for method in METHODS:
        loop = _loop(p, method, x, TIMES)
        grid = getattr(p, method)(x, multi_time=TIMES)
        assert grid.shape == loop.shape == (N, T) and grid.flags.c_contiguous
        assert np.unique(np.round(loop, 9), axis=0).shape[0] == N and np.unique(np.round(loop.T, 9), axis=0).shape[0] == T
        assert np.allclose(grid, loop, rtol=1e-9, atol=0)
        sub = getattr(p, method)(x[64:70], multi_time=TIMES[[3, 1, 4, 0]])      # 6 x 130 x 4 < 2^16: the loop
        assert np.allclose(grid[64:70][:, [3, 1, 4, 0]], sub, rtol=1e-9, atol=0)


def test_the_grid_route_is_taken(calls):
    """One predict_variance_grid call and no per-time call (fails without the grid: T calls per quantity)."""
    m = 130
    x = _problem(m)[1]
    for route in ("std", "cs"):
        p = _predictor(m, route)[0]
        for method, n_grid in (("uncertainty", 1), ("covariance", 2), ("mean_covariance", 3)):
            getattr(p, method)(x, multi_time=TIMES)
            assert calls == {"predict_covariance": 0, "predict_mean_covariance": 0, "predict_variance_grid": n_grid}, method
        calls["predict_variance_grid"] = 0
    # the budget attribute reaches the entry
    assert set(seen_budgets) == {0}
    p._GRID_VARIANCE_DOUBLES = tiny_budget(m, 7)
    try:
        p.uncertainty(x, multi_time=TIMES)
    finally:
        p._GRID_VARIANCE_DOUBLES = 0
    assert seen_budgets[-1] == tiny_budget(m, 7)


def test_fallbacks_keep_the_loop(calls):
    from mellon_amd import cov
    from mellon_amd.base_predictor import PredictorTime
    m = 130
    c, x, L, std, K, kxx, W7, Cs = _problem(m)
    p = _predictor(m, "dense7")[0]

    def same_as_loop(pred, xq, times, **kw):
        for method in METHODS:
            assert np.array_equal(getattr(pred, method)(xq, multi_time=times, **kw), _loop(pred, method, xq, times, **kw))
        assert calls["predict_variance_grid"] == 0

    same_as_loop(p, x[:40], TIMES[:3], diag=False)                # T full matrices
    assert p.covariance(x[:40], multi_time=TIMES[:3], diag=False).shape == (40, 3, 40)
    same_as_loop(p, x, TIMES[:1])                                 # one time is not a grid
    small = PredictorTime(_tree(), c[:20], np.ones(20), 0.0)      # 12 x 20 x 3 < 2^16
    small.L, small.W = np.linalg.cholesky(L[:20] @ L[:20].T + 1e-3 * np.eye(20)), np.array(W7[:20])
    same_as_loop(small, x[:12], TIMES[:3])
    mixed = PredictorTime(cov.Matern52(2.6, active_dims=slice(None, -1)) + cov.Matern52(1.3, active_dims=-1), c,
                          np.ones(m), 0.0)                        # a tree that does not separate
    mixed.L, mixed.W = np.array(L), np.array(W7)
    same_as_loop(mixed, x, TIMES)
    two = PredictorTime(_tree(), c, np.ones((m, 2)), 0.0)         # 2-D weights
    two.L, two.W = np.array(L), np.array(W7)
    same_as_loop(two, x, TIMES)
    # the predictor's own errors, as the single-time call words them
    bare = PredictorTime(_tree(), c, np.ones(m), 0.0)
    for method, text in (("covariance", "without covariance"), ("mean_covariance", "without uncertainty"),
                         ("uncertainty", "without covariance")):
        with pytest.raises(ValueError, match=text) as single:
            getattr(bare, method)(x, time=1.0)
        with pytest.raises(ValueError, match=text) as multi:
            getattr(bare, method)(x, multi_time=TIMES)
        assert str(single.value) == str(multi.value)
    only_l = PredictorTime(_tree(), c, np.ones(m), 0.0)
    only_l.L = np.array(L)
    with pytest.raises(ValueError, match="without uncertainty"):
        only_l.uncertainty(x, multi_time=TIMES)
    per_feature = PredictorTime(_tree(), c, np.ones(m), 0.0)
    per_feature.L, per_feature.per_feature_sigma = np.array(L), True
    with pytest.raises(ValueError, match="per-feature sigma"):
        per_feature.covariance(x, multi_time=TIMES)
    assert calls["predict_variance_grid"] == 0
    assert per_feature.covariance(x, multi_time=TIMES, noise_free=True).shape == (N, T) and calls["predict_variance_grid"] == 1
    for method in METHODS:
        with pytest.raises(ValueError, match="both"):
            getattr(p, method)(x, time=1.0, multi_time=TIMES)


@pytest.fixture(scope="module")
def cells():
    rng = np.random.default_rng(5)
    times = np.repeat(np.arange(4.0), 100)
    X = rng.normal(size=(400, 3)) @ np.array([[2.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.3, -0.5, 0.8]]) + 0.4 * times[:, None]
    return X, times, np.ascontiguousarray(X[::2][:170])


@pytest.mark.parametrize("optimizer", ["L-BFGS-B", "advi"])
def test_fitted_estimator_end_to_end(cells, optimizer):
    """A fitted TimeSensitiveDensityEstimator (Laplace std, and ADVI's): the std route against the restatement with the loop's
    own deviation as the yardstick, and the same predictor after a JSON round trip (general W) against the std route."""
    import mellon_amd
    from mellon_amd.base_predictor import Predictor
    X, times, xq = cells
    est = mellon_amd.TimeSensitiveDensityEstimator(n_landmarks=70, ls_time=1.3, predictor_with_uncertainty=True,
                                                   optimizer=optimizer).fit(X, times)
    p = est.predict
    mt = np.linspace(0.25, 2.75, 9)
    m = p.centers.shape[0]
    assert xq.shape[0] * m * mt.size >= 1 << 16 and p._grid_std() is not None
    state, tleaf = p.cov_func.left, p.cov_func.right
    assert type(state).__name__ == "Matern52" and type(tleaf).__name__ == "Matern52"
    K, kxx = vr.product_kernel(xq, mt, p.centers, ls_state=float(state.ls), ls_time=float(tleaf.ls))
    ref = {k: v.reshape(xq.shape[0], mt.size)
           for k, v in vr.variances(K, kxx, L=p.L, std=p._uncertainty_std[2]).items()}
    q = Predictor.from_json_str(p.to_json())
    assert q._grid_std() is None and np.array_equal(q.W, p.W)
    for method in METHODS:
        r, S = _ref_and_scale(ref, method)
        e_loop = _e(_loop(p, method, xq, mt), r, S)
        bound = 4 * max(e_loop, m * EPS)
        grid = getattr(p, method)(xq, multi_time=mt)
        e_grid = _e(grid, r, S)
        general = getattr(q, method)(xq, multi_time=mt)
        e_general = float((np.abs(general - grid) / S).max())
        print(f"{optimizer} {method:16s} e_grid {e_grid:.2e} e_loop {e_loop:.2e} |general - std| / S {e_general:.2e} "
              f"bound {bound:.2e}")
        assert grid.shape == (xq.shape[0], mt.size)
        assert e_grid <= bound and e_general <= bound, (method, e_grid, e_general, e_loop)


def test_entry_argument_checks():
    from mellon_amd import _lib
    from mellon_amd.base_cov import split_state_time
    m = 130
    c, x, L, std, K, kxx, W7, Cs = _problem(m)
    ctx = _lib.default_context()
    state, tleaf = split_state_time(_tree(), 4)
    xq = np.concatenate([x, np.zeros((N, 1))], axis=1)
    S, _ = ctx.leaf_factors(tleaf, TIMES.reshape(-1, 1), np.ascontiguousarray(c[:, -1:]))
    kdiag = np.ones(T)
    with pytest.raises(_lib.MellonHipError, match="exclude"):
        ctx.predict_variance_grid(state, xq, c, S, kdiag, L, W=W7, std=std)
    with pytest.raises(_lib.MellonHipError, match="no output"):
        ctx.predict_variance_grid(state, xq, c, S, kdiag, L, std=std, want=())
    with pytest.raises(_lib.MellonHipError, match="needs W or std"):
        ctx.predict_variance_grid(state, xq, c, S, kdiag, L, want="mcov")
    with pytest.raises(ValueError):
        ctx.predict_variance_grid(state, xq, c, S[:, :-1], kdiag, L, want="cov")
    empty = ctx.predict_variance_grid(state, xq[:0], c, S, kdiag, L, std=std)
    assert isinstance(empty, tuple) and all(a.shape == (0, T) for a in empty)
    one = ctx.predict_variance_grid(state, xq, c, S, kdiag, L, want="cov")
    assert one.shape == (N, T)
