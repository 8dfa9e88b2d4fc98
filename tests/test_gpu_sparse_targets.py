"""FunctionEstimator on sparse (CSR) targets on a real MI355X (-m gpu): mln_sparse_solve_csr builds y - mu one row panel
at a time from the CSR arrays and feeds the panels to the GEMM of the dense route.

Gates (set by tests/test_gpu_estimators.py::test_function_estimator_vs_oracle for this very solve):
    sparse fit vs dense fit of the same numbers on the same build   rel_max < 1e-9   (two summation orders of one product)
    against the oracle's landmark conditional on the dense y         rel_max < 1e-6
"""
import tracemalloc
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import mellon_oracle as mo

pytestmark = pytest.mark.gpu

D, M, LS, SIGMA = 3, 30, 1.0, 0.4
SAME, ORACLE = 1e-9, 1e-6


def rel_max(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.fixture(scope="module")
def mellon():
    import mellon_amd
    return mellon_amd


@pytest.fixture(scope="module")
def xu():
    return np.random.default_rng(1).normal(size=(M, D))


@pytest.fixture(scope="module")
def xq():
    return np.random.default_rng(2).normal(size=(20, D))


def cells(n, seed=0):
    return np.random.default_rng(seed).normal(size=(n, D))


def sparse_y(n, p, density=0.05, seed=3):
    rng = np.random.default_rng(seed)
    return sp.random(n, p, density=density, format="csr", random_state=rng, data_rvs=rng.standard_normal)


def conditionals(mellon, x, xu, Y, mu, sigma=SIGMA, **kw):
    """The landmark conditional of the CSR targets and of the same numbers dense."""
    from mellon_amd.conditional import LandmarksConditional
    from mellon_amd.validation import CSRTargets, validate_targets
    cov = mellon.cov.Matern52(LS)
    holder = validate_targets(Y, "y")
    assert isinstance(holder, CSRTargets)
    sparse = LandmarksConditional(x, xu, holder, mu, cov, sigma=sigma, **kw)
    dense = LandmarksConditional(x, xu, Y.toarray(), mu, cov, sigma=sigma, **kw)
    return sparse, dense


def check_case(mellon, x, xu, xq, Y, mu, sigma=SIGMA, oracle=True):
    sparse, dense = conditionals(mellon, x, xu, Y, mu, sigma)
    ws, wd = np.asarray(sparse.weights), np.asarray(dense.weights)
    assert ws.shape == wd.shape == (M, Y.shape[1])
    ps, pd = sparse(xq), dense(xq)
    print(f"n={x.shape[0]} p={Y.shape[1]} mu={mu}: weights {rel_max(ws, wd):.2e} predictions {rel_max(ps, pd):.2e}", end="")
    assert rel_max(ws, wd) < SAME and rel_max(ps, pd) < SAME
    if oracle:
        ref = mo.function_fit(x, Y.toarray(), sigma, mu=mu, landmarks=xu, ls=LS)
        print(f" vs oracle {rel_max(ps, ref(xq)):.2e}", end="")
        assert rel_max(ps, ref(xq)) < ORACLE
    print()
    return sparse, dense


# ---- panel edges ---------------------------------------------------------------------------------------------------
P_EDGE = 16384        # columns at which a panel holds a few hundred rows


def test_panel_geometry(mellon):
    from mellon_amd import _lib
    assert _lib.csr_panel_rows(P_EDGE) == _lib.CSR_PANEL_BYTES // (8 * P_EDGE) and 128 <= _lib.csr_panel_rows(P_EDGE) <= 1024
    assert _lib.csr_panel_rows(70000) == 64


@pytest.mark.parametrize("mu", [0.0, 0.7])
@pytest.mark.parametrize("which", ["1", "63", "P-1", "P", "P+1", "2P+17"])
def test_panel_edges_in_rows(mellon, xu, xq, which, mu):
    from mellon_amd import _lib
    P = _lib.csr_panel_rows(P_EDGE)
    n = {"1": 1, "63": 63, "P-1": P - 1, "P": P, "P+1": P + 1, "2P+17": 2 * P + 17}[which]
    check_case(mellon, cells(n), xu, xq, sparse_y(n, P_EDGE), mu)


@pytest.mark.parametrize("mu", [0.0, 0.7])
@pytest.mark.parametrize("p", [1, 2, 127, 128, 129])
def test_column_counts(mellon, xu, xq, p, mu):
    check_case(mellon, cells(300), xu, xq, sparse_y(300, p), mu)


@pytest.mark.parametrize("mu", [0.0, 0.7])
def test_panel_floor_of_64_rows(mellon, xu, xq, mu):
    from mellon_amd import _lib
    p = 70000
    assert _lib.csr_panel_rows(p) == 64
    check_case(mellon, cells(150), xu, xq, sparse_y(150, p), mu)        # panels of 64, 64 and 22 rows


# ---- patterns ------------------------------------------------------------------------------------------------------
def pattern(name, n=200, p=50):
    rng = np.random.default_rng(7)
    A = rng.normal(size=(n, p)) * (rng.random((n, p)) < 0.05)
    if name == "one dense row":
        A[:] = 0.0
        A[n // 2] = rng.normal(size=p)
    elif name == "empty first and last row":
        A[0] = A[-1] = 0.0
    elif name == "empty first and last column":
        A[:, 0] = A[:, -1] = 0.0
    elif name == "last column only":
        A[:, :-1] = 0.0
        A[:, -1] = rng.normal(size=n)
    Y = sp.csr_matrix(A)
    if name == "explicit zeros":
        Y.data[::3] = 0.0            # stored values that are zero
        assert Y.nnz == np.count_nonzero(A) and np.count_nonzero(Y.data) < Y.nnz
    return Y


@pytest.mark.parametrize("mu", [0.0, 0.7])
@pytest.mark.parametrize("name", ["one dense row", "empty first and last row", "empty first and last column",
                                  "explicit zeros", "last column only"])
def test_patterns(mellon, xu, xq, name, mu):
    check_case(mellon, cells(200), xu, xq, pattern(name), mu)


@pytest.mark.parametrize("mu", [0.0, 0.7])
def test_all_zero_targets(mellon, xu, xq, mu):
    """nnz = 0: every panel is the fill alone.  With mu = 0 both routes multiply by exact zeros, so the weights are
    exactly the dense route's (zeros); with mu != 0 the one panel holds the dense route's R element for element."""
    x = cells(200)
    Y = sp.csr_matrix((200, 50))
    sparse, dense = conditionals(mellon, x, xu, Y, mu)
    if mu == 0.0:
        assert np.array_equal(np.asarray(sparse.weights), np.asarray(dense.weights))
        assert not np.any(np.asarray(sparse.weights))
    else:
        assert rel_max(np.asarray(sparse.weights), np.asarray(dense.weights)) < SAME
        ref = mo.function_fit(x, np.zeros((200, 50)), SIGMA, mu=mu, landmarks=xu, ls=LS)
        assert rel_max(sparse(xq), ref(xq)) < ORACLE


# ---- noise models --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [3, 40])
def test_per_output_sigma(mellon, xu, xq, levels):
    """3 levels: one Cholesky per run of equal sigma; 40 distinct levels: the spectral branch (above 32)."""
    p = 12 if levels == 3 else 40
    sigma = np.repeat([0.3, 0.5, 0.8], 4) if levels == 3 else np.linspace(0.2, 1.0, 40)
    x = cells(400)
    for mu in (0.0, 0.7):
        sparse, dense = check_case(mellon, x, xu, xq, sparse_y(400, p, density=0.2), mu, sigma=sigma)
        assert sparse.per_feature_sigma and dense.per_feature_sigma
    row = check_case(mellon, x, xu, xq, sparse_y(400, p, density=0.2), 0.7, sigma=sigma[None, :], oracle=False)[0]   # (1, p)
    assert np.array_equal(np.asarray(row.weights), np.asarray(sparse.weights))


def test_with_uncertainty_factors(mellon, xu, xq):
    x, Y = cells(400), sparse_y(400, 9, density=0.2)
    sparse, dense = conditionals(mellon, x, xu, Y, 0.7, with_uncertainty=True)
    assert rel_max(np.asarray(sparse.weights), np.asarray(dense.weights)) < SAME
    assert rel_max(np.asarray(sparse.L), np.asarray(dense.L)) < SAME
    assert rel_max(np.asarray(sparse.Cs), np.asarray(dense.Cs)) < SAME
    for kw in (dict(noise_free=True), dict(), dict(diag=False)):
        assert rel_max(sparse.covariance(xq, **kw), dense.covariance(xq, **kw)) < SAME
    ref = mo.function_fit(x, Y.toarray(), SIGMA, mu=0.7, landmarks=xu, ls=LS, with_uncertainty=True)
    assert rel_max(sparse.covariance(xq), ref.covariance(xq)) < ORACLE
    # a noisy landmark conditional carries no mean covariance W: `uncertainty` refuses on both routes alike
    for pred in (sparse, dense):
        with pytest.raises(ValueError, match="without uncertainty"):
            pred.uncertainty(xq)


# ---- the estimator: sparse route and the dense fallbacks -----------------------------------------------------------
def user_matern52(mellon):
    class UserMatern52(mellon.base_cov.Covariance):
        """A user's own kernel written in NumPy: evaluated block by block, never lowered to a device program."""

        def __init__(self, ls=1.0):
            super().__init__()
            self.ls = ls

        def k(self, x, y):
            sq = (x * x).sum(1)[:, None] - 2.0 * x @ y.T + (y * y).sum(1)[None, :] + 1e-12
            r = np.sqrt(5.0) * np.sqrt(np.maximum(sq, 0.0)) / self.ls
            return (r + r * r / 3.0 + 1.0) * np.exp(-r)

    return UserMatern52


def test_estimator_fit_keeps_the_callers_object(mellon, xu, xq):
    x, Y = cells(300), sparse_y(300, 6, density=0.2)
    est = mellon.FunctionEstimator(sigma=SIGMA, landmarks=xu, ls=LS, mu=0.7)
    out = est.fit_predict(x, Y, xq)
    assert est.y is Y and out.shape == (20, 6)
    ref = mellon.FunctionEstimator(sigma=SIGMA, landmarks=xu, ls=LS, mu=0.7).fit_predict(x, Y.toarray(), xq)
    assert rel_max(out, ref) < SAME
    assert rel_max(out, mo.function_fit(x, Y.toarray(), SIGMA, mu=0.7, landmarks=xu, ls=LS)(xq)) < ORACLE
    for fmt in (sp.csc_matrix, sp.coo_array, sp.csr_array):
        assert np.array_equal(mellon.FunctionEstimator(sigma=SIGMA, landmarks=xu, ls=LS, mu=0.7).fit_predict(x, fmt(Y), xq), out)
    assert rel_max(est.loo_residuals_squared(), est.loo_residuals_squared(x, Y.toarray())) < SAME


@pytest.mark.parametrize("route", ["obs_variance", "full", "y_is_mean", "sigma (n, p)", "python kernel"])
def test_fallbacks_give_the_dense_answer(mellon, xu, xq, route):
    n, p = 300, 6
    x, Y = cells(n), sparse_y(n, p, density=0.2)
    kw = dict(sigma=SIGMA, landmarks=xu, ls=LS, mu=0.3)
    if route == "obs_variance":
        kw["obs_variance"] = True
    elif route == "full":
        kw = dict(sigma=SIGMA, gp_type="full", ls=LS, mu=0.3)
    elif route == "y_is_mean":
        kw["y_is_mean"] = True
    elif route == "sigma (n, p)":
        kw["sigma"] = 0.2 + np.random.default_rng(4).random((n, p))
    elif route == "python kernel":
        kw = dict(sigma=SIGMA, landmarks=xu, cov_func=user_matern52(mellon)(LS), mu=0.3)
    es = mellon.FunctionEstimator(**kw).fit(x, Y)
    ed = mellon.FunctionEstimator(**kw).fit(x, Y.toarray())
    assert es.y is Y
    assert rel_max(np.asarray(es.predict.weights), np.asarray(ed.predict.weights)) < SAME
    assert rel_max(es.predict(xq), ed.predict(xq)) < SAME
    if route == "obs_variance":
        assert rel_max(es.get_obs_variance(xq), ed.get_obs_variance(xq)) < SAME
        assert rel_max(es.loo_residuals_squared(), ed.loo_residuals_squared()) < SAME
        assert rel_max(es.leverage(), ed.leverage()) < SAME


def test_multi_fit_predict_takes_genes_by_cells(mellon, xu, xq):
    x = cells(300)
    Yg = sparse_y(7, 300, density=0.2)                   # functions (genes) as rows
    kw = dict(sigma=SIGMA, landmarks=xu, ls=LS, mu=0.3)
    es = mellon.FunctionEstimator(**kw)
    out = es.multi_fit_predict(x, Yg, xq)
    assert out.shape == (7, 20)
    assert rel_max(out, mellon.FunctionEstimator(**kw).multi_fit_predict(x, Yg.toarray(), xq)) < SAME
    assert rel_max(out.T, mo.function_fit(x, Yg.toarray().T, SIGMA, mu=0.3, landmarks=xu, ls=LS)(xq)) < ORACLE


def test_two_sparse_fits_give_the_same_bits(mellon, xu):
    from mellon_amd import _lib
    p = 16384
    n = 2 * _lib.csr_panel_rows(p) + 17
    x, Y = cells(n), sparse_y(n, p)
    a = np.asarray
    from mellon_amd.conditional import LandmarksConditional
    from mellon_amd.validation import validate_targets
    cov = mellon.cov.Matern52(LS)
    w1 = a(LandmarksConditional(x, xu, validate_targets(Y, "y"), 0.7, cov, sigma=SIGMA).weights)
    w2 = a(LandmarksConditional(x, xu, validate_targets(Y.tocsc(), "y"), 0.7, cov, sigma=SIGMA).weights)
    assert np.array_equal(w1, w2)


# ---- no dense copy -------------------------------------------------------------------------------------------------
def test_no_dense_copy_on_host_or_device(mellon):
    """n = 20 000, p = 4096: the dense y would be 655 MB.  Everything the sparse fit drew from the driver (the allocator's
    live + cached bytes after a release) and the peak of the host allocations over the call stay below half of that:
    the K buffer, the CSR arrays, the k-split partials and one panel are under 40 MB plus CSR_PANEL_BYTES."""
    from mellon_amd import _lib
    n, p, m = 20000, 4096, 64
    assert _lib.CSR_PANEL_BYTES <= 128 << 20
    dense_bytes = 8 * n * p
    x = cells(n)
    lm = np.random.default_rng(5).normal(size=(m, D))
    Y = sparse_y(n, p, density=0.02)
    est = mellon.FunctionEstimator(sigma=SIGMA, landmarks=lm, ls=LS)
    _lib.default_context().synchronize()
    _lib.release_cached_memory()
    before = _lib.alloc_stats()
    tracemalloc.start()
    est.fit(x, Y)
    host_peak = tracemalloc.get_traced_memory()[1]
    tracemalloc.stop()
    after = _lib.alloc_stats()
    drawn = after["live_bytes"] + after["cached_bytes"]
    print(f"device: {drawn / 1e6:.1f} MB live + cached after the fit ({(before['live_bytes'] + before['cached_bytes']) / 1e6:.1f} MB "
          f"before); host peak {host_peak / 1e6:.1f} MB; dense y {dense_bytes / 1e6:.1f} MB")
    assert drawn < dense_bytes // 2
    assert host_peak < dense_bytes // 2
    assert np.asarray(est.predict.weights).shape == (m, p) and np.all(np.isfinite(est.predict.weights))
    # the same numbers through the dense route, on a slice of the outputs small enough to hold
    cols = slice(1000, 1016)
    ref = mellon.FunctionEstimator(sigma=SIGMA, landmarks=lm, ls=LS).fit(x, Y[:, cols].toarray())
    assert rel_max(np.asarray(est.predict.weights)[:, cols], np.asarray(ref.predict.weights)) < SAME


# ---- refusals before any launch ------------------------------------------------------------------------------------
def small_csr():
    indptr = np.array([0, 2, 2, 3, 5], dtype=np.int64)
    indices = np.array([0, 3, 1, 2, 4], dtype=np.int32)
    data = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    return SimpleNamespace(indptr=indptr, indices=indices, data=data, shape=(4, 5))


@pytest.mark.parametrize("defect", ["index == p", "negative index", "decreasing indptr", "indptr[-1] != nnz",
                                    "repeated index", "unsorted index", "indptr[0] != 0", "non-finite", "per-cell sigma"])
def test_malformed_csr_is_refused(mellon, defect):
    from mellon_amd import _lib
    ctx = _lib.default_context()
    desc = mellon.cov.Matern52(LS).lower(D)
    x, lm = cells(4), cells(3, seed=9)
    y, sigma, kind = small_csr(), 0.4, ctx.SIGMA_SCALAR
    W = ctx.sparse_solve_csr(desc, x, lm, y, 0.0, sigma, kind, 1e-6)          # the well-formed matrix is served
    assert W.shape == (3, 5) and np.all(np.isfinite(W))
    if defect == "index == p":
        y.indices[1] = 5
    elif defect == "negative index":
        y.indices[2] = -1
    elif defect == "decreasing indptr":
        y.indptr[:] = [0, 3, 2, 3, 5]
    elif defect == "indptr[-1] != nnz":
        y.indptr[-1] = 4
    elif defect == "repeated index":
        y.indices[:2] = [3, 3]
    elif defect == "unsorted index":
        y.indices[:2] = [3, 0]
    elif defect == "indptr[0] != 0":
        y.indptr[0] = 1
    elif defect == "non-finite":
        y.data[3] = np.nan
    elif defect == "per-cell sigma":
        sigma, kind = np.full(4, 0.4), ctx.SIGMA_PER_CELL
    with pytest.raises(_lib.MellonHipError, match=f"error {_lib.MLN_ERR_ARG}"):
        ctx.sparse_solve_csr(desc, x, lm, y, 0.0, sigma, kind, 1e-6)
