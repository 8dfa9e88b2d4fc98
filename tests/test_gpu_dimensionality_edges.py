"""Edges of the dimensionality kernels on a real MI355X (-m gpu): exact ties and tile edges of the k-NN search (k_knn),
every bitonic sort size, LDS feature stage and equidistant neighbourhood of the local dimension (k_local_dim), and all
ten k_dim_objective<CPT, R, HESS> instantiations with multi-term lanes and special functions over a wide range of D.
Each device result is checked against an independent fp64 (or longdouble / mpmath) reference of the same operation."""
import numpy as np
import pytest
from scipy.optimize import minimize

import dim_restatement as dr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from mellon_amd import _lib
    return _lib.default_context()


def exact_knn(x, y, k, exclude=False, offset=0):
    """Brute force in difference form, every pair; ties go to the smaller index (stable argsort)."""
    d2 = np.zeros((x.shape[0], y.shape[0]))
    for f in range(x.shape[1]):
        d2 += (x[:, f, None] - y[None, :, f]) ** 2
    if exclude:
        rows = np.arange(x.shape[0])
        cols = rows + offset
        ok = (cols >= 0) & (cols < y.shape[0])
        d2[rows[ok], cols[ok]] = np.inf
    o = np.argsort(d2, axis=1, kind="stable")[:, :k]
    return np.sqrt(np.take_along_axis(d2, o, axis=1)), o


# ---- k-NN ---------------------------------------------------------------------------------------------------------
def _lattice(shape):
    return np.stack(np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij"), -1).reshape(-1, len(shape))


@pytest.mark.parametrize("shape", [(50, 50), (14, 14, 14)])
def test_knn_exact_ties_on_a_lattice(ctx, shape):
    """Squared distances are exact integers: distances bit-equal, and the index at EVERY position is the smaller-index
    tie rule's, with tie groups straddling the 64-row candidate tiles and the k-th place."""
    x = _lattice(shape)
    for exclude in (False, True):
        ref_d, ref_i = exact_knn(x, x, 64, exclude=exclude)
        for k in (1, 4, 10, 63, 64):
            dist, idx = ctx.knn(x, k, exclude_self=exclude)
            assert np.array_equal(dist, ref_d[:, :k]), (k, exclude, np.abs(dist - ref_d[:, :k]).max())
            assert np.array_equal(idx, ref_i[:, :k]), (k, exclude, np.argwhere(idx != ref_i[:, :k])[:5])


def test_knn_all_identical_rows(ctx):
    x = np.full((200, 5), 0.37)
    for k in (1, 10, 64):
        dist, idx = ctx.knn(x, k)
        assert np.all(dist == 0) and np.array_equal(idx, np.broadcast_to(np.arange(k), (200, k)))
        dist, idx = ctx.knn(x, k, exclude_self=True)
        want = np.array([[j for j in range(k + 1) if j != i][:k] for i in range(200)])
        assert np.all(dist == 0) and np.array_equal(idx, want)


def _check_random(ctx, x, y, k, exclude=False, offset=0):
    dist, idx = ctx.knn(x, k, y=y, exclude_self=exclude, self_offset=offset)
    ref_d, ref_i = exact_knn(x, y, k, exclude=exclude, offset=offset)
    assert np.all(np.abs(dist - ref_d) <= 1e-13 * ref_d), np.abs(dist - ref_d).max()
    assert np.array_equal(idx, ref_i)


@pytest.mark.parametrize("n", [63, 64, 65, 127, 129])
def test_knn_tile_and_feature_stage_edges(ctx, n):
    rng = np.random.default_rng(n)
    for m in (63, 64, 65, 127, 129):
        for d in (15, 16, 17, 32, 33):
            y = rng.normal(size=(m, d))
            x = rng.normal(size=(n, d))
            _check_random(ctx, x, y, min(m, 64))
            # a query set that overlaps the candidates: x = y[off : off + n] (perturbed), the pair (i, i + off) skipped
            off = (m - 1) // 3
            xs = y[off:off + n] + 1e-3 * rng.normal(size=(min(n, m - off), d))
            _check_random(ctx, xs, y, min(m - 1, 64), exclude=True, offset=off)


def test_knn_fewer_candidates_than_a_tile_and_offsets_outside(ctx):
    rng = np.random.default_rng(5)
    y = rng.normal(size=(40, 7))
    x = rng.normal(size=(200, 7))                 # m < 64 < n
    _check_random(ctx, x, y, 40)
    # the skipped column i + offset lies in [0, m) for 40 of the queries, for 20 of them, or for none
    for off in (-100, -180, 10_000):
        _check_random(ctx, x, y, 39, exclude=True, offset=off)


def test_knn_difference_form_precision(ctx):
    """Rows at 1e6 with spread 1e-3: a Gram form (|x|^2 + |y|^2 - 2 x.y) loses every digit; the difference form keeps
    the distances to 1e-13 of an extended-precision brute force."""
    rng = np.random.default_rng(6)
    x = 1e6 + 1e-3 * rng.normal(size=(500, 8))
    dist, idx = ctx.knn(x, 16, exclude_self=True)
    xl = x.astype(np.longdouble)
    d2 = np.zeros((500, 500), dtype=np.longdouble)
    for f in range(8):
        d2 += (xl[:, f, None] - xl[None, :, f]) ** 2
    np.fill_diagonal(d2, np.inf)
    o = np.argsort(d2, axis=1, kind="stable")[:, :16]
    ref = np.sqrt(np.take_along_axis(d2, o, axis=1))
    assert np.all(np.abs(dist.astype(np.longdouble) - ref) <= 1e-13 * ref), float(np.max(np.abs(dist - ref) / ref))
    assert np.array_equal(idx, o)


def test_knn_device_inputs_match_host_inputs(ctx):
    rng = np.random.default_rng(8)
    x = rng.normal(size=(300, 21))
    y = rng.normal(size=(150, 21))
    for kw in ({}, {"y": y}, {"y": y, "exclude_self": True, "self_offset": 3}):
        dh, ih = ctx.knn(x, 33, **kw)
        dkw = dict(kw)
        if "y" in kw:
            dkw["y"] = ctx.to_device(y)
        dd, idd = ctx.knn(ctx.to_device(x), 33, **dkw)
        assert np.array_equal(dh.view(np.int64), dd.view(np.int64)) and np.array_equal(ih, idd)


# ---- local dimension ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 31, 32, 33, 65, 100])
def test_local_dim_sort_sizes_and_feature_stages(ctx, d):
    """k = 2 ... 64: bitonic sorts of 2 ... 2048 entries; d across the 32-feature LDS stages."""
    rng = np.random.default_rng(d)
    x = rng.normal(size=(300, d)) * rng.uniform(0.5, 2.0, size=d)
    for k in (2, 3, 32, 45, 46, 64):
        nbr = np.stack([rng.choice(300, size=k, replace=False) for _ in range(24)])
        got = ctx.local_dimensionality(x, nbr)
        want = dr.local_dimensionality(x, neighbor_idx=nbr)
        if k == 2:
            assert np.array_equal(got, want) and np.all(got == 0)
        else:
            np.testing.assert_allclose(got, want, rtol=1e-10, atol=0)


def test_local_dim_repeated_and_negative_indices(ctx):
    rng = np.random.default_rng(3)
    x = rng.normal(size=(120, 9))
    nbr = np.stack([rng.choice(120, size=20, replace=False) for _ in range(10)])
    neg = nbr - 120                                   # the same rows, counted from the end
    np.testing.assert_array_equal(ctx.local_dimensionality(x, neg), ctx.local_dimensionality(x, nbr))
    mixed = np.where(rng.uniform(size=nbr.shape) < 0.5, neg, nbr)
    np.testing.assert_allclose(ctx.local_dimensionality(x, mixed), dr.local_dimensionality(x, neighbor_idx=mixed),
                               rtol=1e-10)
    rep = nbr.copy()
    rep[::2, 7] = rep[::2, 3]                         # a repeated row: a zero pair distance
    got = ctx.local_dimensionality(x, rep)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = dr.local_dimensionality(x, neighbor_idx=rep)
    assert np.all(np.isnan(got[::2])) and np.all(np.isnan(want[::2]))
    np.testing.assert_allclose(got[1::2], want[1::2], rtol=1e-10)


@pytest.mark.parametrize("k", [3, 4, 10, 30, 64])
def test_local_dim_equidistant_neighbourhoods_match_lstsq(ctx, k):
    """Every pair distance equal (exactly, or to rounding): [log dist, 1] has rank 1 and lstsq returns its minimum-norm
    solution, which the closed-form slope alone does not."""
    rng = np.random.default_rng(k)
    cases = [dr.one_hot_rows(k), np.pad(dr.one_hot_rows(k), ((0, 0), (0, 100 - k))), 3.0 * dr.one_hot_rows(k)]
    cases += [dr.rotated_simplex(k, s) * sc for s, sc in ((1, 1.0), (2, 0.01), (3, 50.0))]
    for x in cases:
        nbrs = np.stack([np.arange(k), rng.permutation(k), rng.permutation(k)])
        got = ctx.local_dimensionality(x, nbrs)
        want = np.array([np.linalg.lstsq(np.stack([np.log(np.sort(nd)), np.ones_like(nd)], 1),
                                         np.log(np.arange(1, nd.size + 1)), rcond=None)[0][0]
                         for nd in (dr.pair_distances(x[i]) for i in nbrs)])
        assert np.all(np.isfinite(got))
        np.testing.assert_allclose(got, want, rtol=1e-10, atol=0)
    # well-conditioned neighbourhoods of the same sizes, for contrast
    x = rng.normal(size=(k + 20, 6))
    nbrs = np.stack([rng.choice(k + 20, size=k, replace=False) for _ in range(5)])
    np.testing.assert_allclose(ctx.local_dimensionality(x, nbrs), dr.local_dimensionality(x, neighbor_idx=nbrs),
                               rtol=1e-10)


# ---- dimensionality objective -------------------------------------------------------------------------------------
def _check_objective(fit, L, ell, z, mu_dim, mu_dens, hess=True):
    fit.set_dim_likelihood(ell, mu_dim, mu_dens)
    want = dr.dim_loss(z, L, ell, mu_dim, mu_dens)
    gw, hw = dr.dim_grad_hess(z, L, ell, mu_dim, mu_dens)
    if hess:
        loss, g, h = fit.dim_objective(z, with_hess=True)
        np.testing.assert_allclose(h, hw, rtol=1e-9, atol=1e-9 * np.abs(hw).max())
        loss2, g2 = fit.dim_objective(z)                  # the Hessian's second pass leaves the first one's results alone
        assert loss2 == loss and np.array_equal(g2, g)
    else:
        loss, g = fit.dim_objective(z)
    assert abs(loss - want) <= 1e-11 * abs(want), (loss, want)
    np.testing.assert_allclose(g, gw, rtol=1e-9, atol=1e-9 * np.abs(gw).max())


# m -> CPT = ceil(pad16(m) / 1024): 1 1 | 2 2 | 3 3 | 4 4 | 5 5; R = 2 for CPT <= 3, 1 above
CPT_BANDS = [1023, 1024, 1025, 2048, 2049, 3072, 3073, 4096, 4097, 5120]


@pytest.mark.parametrize("m", CPT_BANDS)
def test_dim_objective_cpt_bands_terms_per_lane_and_small_n(ctx, m):
    """Every <CPT, R, HESS>; k = 1, 32, 33, 64 (with R = 2 and k >= 33 a lane holds two terms and a row straddles the
    two); n = 1 and 3 (fewer rows than workgroups), n = 513 (odd, and workgroups with no step).  The same fit takes the
    four k in turn: set_dim_likelihood reallocates its buffer each time."""
    from mellon_amd._lib import Fit
    rng = np.random.default_rng(m)
    for n in (1, 3, 513):
        L = rng.normal(size=(n, m)) * (0.6 / np.sqrt(m))
        fit = Fit.from_L(ctx, L)
        for k in (1, 32, 33, 64):
            ell = dr.ell_of(np.abs(rng.normal(size=(n, k))) + 0.05)
            z = rng.normal(size=(2, m)) * 0.5
            _check_objective(fit, L, ell, z, 0.3, 1.1)


def test_dim_objective_one_pass_limit_from_L(ctx):
    from mellon_amd._lib import Fit
    rng = np.random.default_rng(0)
    fit = Fit.from_L(ctx, rng.normal(size=(4, 5121)) * 0.01)
    with pytest.raises(NotImplementedError, match="5120"):
        fit.set_dim_likelihood(np.zeros((4, 10)), 0.0, 0.0)


@pytest.mark.parametrize("kind,n,m,k", [("implicit", 2501, 2049, 33), ("sparse_cholesky", 3501, 3073, 64),
                                        ("full", 1025, None, 1), ("implicit", 4511, 4097, 32)])
def test_dim_objective_prepared_fits(ctx, kind, n, m, k):
    from mellon_amd import cov
    rng = np.random.default_rng(n)
    x = rng.normal(size=(n, 3))
    kern = cov.Matern52(1.3)
    xu = None if kind == "full" else x[rng.choice(n, m, replace=False)]
    fit = ctx.fit_prepare(kern.lower(3), x, xu, 1e-6, implicit=(kind == "implicit"))
    L = fit.L()
    ell = dr.ell_of(np.abs(rng.normal(size=(n, k))) + 0.05)
    z = rng.normal(size=(2, fit.m)) * 0.1
    _check_objective(fit, L, ell, z, 0.3, 1.1, hess=kind != "implicit")


def _mp_objective(z, L, ell, mu_dim, mu_dens):
    """The loss, gradient and Hessian diagonal in 30-digit arithmetic on the same fp64 inputs."""
    import mpmath as mp
    mp.mp.dps = 30
    n, m = L.shape
    k = ell.shape[1]
    Lm = [[mp.mpf(float(v)) for v in row] for row in L]
    zm = [[mp.mpf(float(v)) for v in row] for row in z]
    loss = mp.mpf(0)
    c0, c1, h0r, h1r = [], [], [], []
    for i in range(n):
        f0 = mp.fsum(Lm[i][j] * zm[0][j] for j in range(m))
        f1 = mp.fsum(Lm[i][j] * zm[1][j] for j in range(m))
        D = mp.exp(mu_dim + f0)
        xh = D / 2 + 1
        lg, ps, tp = mp.loggamma(xh), mp.digamma(xh), mp.polygamma(1, xh)
        sa = sas = se = sh = mp.mpf(0)
        for j in range(k):
            e_ = mp.mpf(float(ell[i, j]))
            pred = mp.mpf(mu_dens) + f1 + D * e_ - lg
            ex = mp.exp(pred)
            cnt = j + 1
            loss += pred * cnt - ex - mp.loggamma(cnt)
            a = cnt - ex
            s = e_ - ps / 2
            sa += a
            sas += a * s
            se += ex
            sh += ex * s * s + a * tp / 4
        c0.append(-D * sas)
        c1.append(-sa)
        h0r.append(-D * sas + D * D * sh)
        h1r.append(se)
    out_loss = mp.fsum(v * v for row in zm for v in row) / 2 + mp.log(2 * mp.pi) - loss
    g = np.array([[float(zm[r][j] + mp.fsum(Lm[i][j] * c[i] for i in range(n))) for j in range(m)]
                  for r, c in ((0, c0), (1, c1))])
    h = np.array([[float(1 + mp.fsum(Lm[i][j] ** 2 * c[i] for i in range(n))) for j in range(m)]
                  for c in (h0r, h1r)])
    return float(out_loss), g, h


@pytest.mark.parametrize("k", [33, 64])
def test_dim_objective_special_functions_over_D(ctx, k):
    """D from about 0.05 to 500, with rows just below, at and just above D = 10, where lnGamma, psi and psi' of D / 2 + 1
    switch from the recurrence to the asymptotic series; exp(pred) between about e^-6 and e^6."""
    from scipy.special import gammaln
    from mellon_amd._lib import Fit
    rng = np.random.default_rng(k)
    n, m = 64, 40
    mu_dim, mu_dens = 0.25, -0.4                      # (mu_dim + (t - mu_dim) == t exactly for t near log 10)
    ulp = np.spacing(np.log(10.0))                    # no fp64 t has exp(t) == 10: the closest give 10 -+ 1 ulp of 10
    logD = np.concatenate([np.linspace(np.log(0.05), np.log(500.0), n - 8),
                           np.log(10.0) + np.array([-1e-3, -1e-9, -2 * ulp, -ulp, 0.0, ulp, 1e-9, 1e-3])])
    L = 0.01 * rng.normal(size=(n, m))
    L[:, 0] = logD - mu_dim
    L[n - 8:, 1:] = 0.0                               # the D = 10 rows: D = exp(mu_dim + L[i, 0]) alone
    z = 0.3 * rng.normal(size=(2, m))
    z[0, 0] = 1.0
    D = np.exp(mu_dim + L @ z[0])
    log_dens = mu_dens + L @ z[1]
    pred = np.sort(rng.uniform(-6.0, 6.0, size=(n, k)), axis=1)
    ell = (pred - log_dens[:, None] + gammaln(D / 2 + 1)[:, None]) / D[:, None]
    assert 0.04 < D.min() and D.max() < 600 and np.any(D < 10) and np.any(D > 10)
    fit = Fit.from_L(ctx, L)
    fit.set_dim_likelihood(ell, mu_dim, mu_dens)
    loss, g, h = fit.dim_objective(z, with_hess=True)
    want, gw, hw = _mp_objective(z, L, ell, mu_dim, mu_dens)
    assert abs(loss - want) <= 1e-11 * abs(want), (loss, want)
    np.testing.assert_allclose(g, gw, rtol=1e-9, atol=1e-9 * np.abs(gw).max())
    np.testing.assert_allclose(h, hw, rtol=1e-9, atol=1e-9 * np.abs(hw).max())


# ---- estimator ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 33, 64])
def test_estimator_k_end_to_end(k):
    import mellon_amd
    rng = np.random.default_rng(30 + k)
    x = rng.normal(size=(1500, 4))
    est = mellon_amd.DimensionalityEstimator(k=k, n_landmarks=150)
    dim = est.fit_predict(x)
    ref_d, _ = exact_knn(x, x, k, exclude=True)
    assert est.distances.shape == (1500, k)
    np.testing.assert_allclose(est.distances, ref_d, rtol=1e-13, atol=0)
    np.testing.assert_allclose(est.d, dr.local_dimensionality(x), rtol=1e-10)
    L = np.asarray(est.L)
    ell = dr.ell_of(est.distances)
    loss = dr.dim_loss(est.pre_transformation, L, ell, est.mu_dim, est.mu_dens)
    assert abs(est.losses[-1] - loss) <= 1e-9 * abs(loss)
    z0 = dr.initial_dimensionalities(L, est.d, est.mu_dim, est.nn_distances, est.mu_dens)
    # the Ridge start's Gram is the exact integer Gram of K quantised to 2^-23 (gram_i8): the bound of the
    # other Ridge-start checks (test_gpu_ops.py), relative to the largest entry
    assert np.abs(est.initial_value - z0).max() <= 1e-7 * np.abs(z0).max()
    res = minimize(lambda z: (dr.dim_loss(z, L, ell, est.mu_dim, est.mu_dens),
                              dr.dim_grad_hess(z, L, ell, est.mu_dim, est.mu_dens)[0].ravel()),
                   z0.ravel(), jac=True, method="L-BFGS-B", options=dict(maxiter=20000, maxfun=50000, ftol=1e-15, gtol=1e-9))
    zs = res.x.reshape(2, -1)
    want_dim = np.exp(est.mu_dim + L @ zs[0])
    want_dens = est.mu_dens + L @ zs[1]
    assert np.abs(dim - want_dim).max() <= 1e-5 * np.abs(want_dim).max()
    assert np.abs(est.log_density_x - want_dens).max() <= 1e-5 * np.abs(want_dens).max()


def test_estimator_rejects_k_beyond_64():
    import mellon_amd
    x = np.random.default_rng(0).normal(size=(300, 3))
    with pytest.raises(ValueError, match="1 <= k <= 64"):
        mellon_amd.DimensionalityEstimator(k=65).fit(x)


def test_estimator_one_hot_cells_have_a_finite_local_dimension():
    import mellon_amd
    x = np.eye(200)
    est = mellon_amd.DimensionalityEstimator()
    est.prepare_inference(x)
    want = dr.local_dimensionality(x)
    assert np.all(np.isfinite(est.d))
    np.testing.assert_allclose(est.d, want, rtol=1e-10, atol=0)
