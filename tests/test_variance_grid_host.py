"""The longdouble restatement of the predictive variances (variance_restatement.py) against their dense definitions on a
12-landmark problem, and the identity behind the `std` route of the variance grid."""
import numpy as np

import variance_restatement as vr

N, M, T = 9, 12, 4
TIMES = np.linspace(0.25, 2.75, T)


def _problem():
    c, x, L, std = vr.make_problem(N, M, seed=11)
    K, kxx = vr.product_kernel(x, TIMES, c)
    return c, x, L, std, K, kxx


def test_restatement_matches_the_dense_definitions():
    """k** - k^T (L L^T)^-1 k and k^T W W^T k from numpy's dense solves in float64: at m = 12 and cond(L L^T) ~ 1e3 the
    float64 side is good to ~1e-12 relative to k** + k^T (L L^T)^-1 k; 1e-10 leaves two digits."""
    c, x, L, std, K, kxx = _problem()
    rng = np.random.default_rng(3)
    W = rng.normal(size=(M, 5))
    B = rng.normal(size=(M, 3)) * 0.3
    Cs = L @ np.linalg.cholesky(np.eye(M) + B @ B.T)
    r = vr.variances(K, kxx, L=L, W=W)
    assert r["cov"].dtype == np.longdouble and r["cov"].shape == (N * T,)
    K64 = K.astype(np.float64)
    quad = np.einsum("ji,ji->i", K64, np.linalg.solve(L @ L.T, K64))
    cov = float(kxx) - quad
    assert np.abs(cov - r["cov"].astype(np.float64)).max() <= 1e-10 * (float(kxx) + quad.max())
    assert np.abs((float(kxx) + quad) - r["S_cov"].astype(np.float64)).max() <= 1e-10 * (float(kxx) + quad.max())
    mc = np.square(W.T @ K64).sum(axis=0)
    assert np.abs(mc - r["mcov"].astype(np.float64)).max() <= 1e-10 * mc.max()
    assert np.array_equal(r["S_mcov"], r["mcov"])
    # the Cs term: + k^T (Cs Cs^T)^-1 k
    rc = vr.variances(K, kxx, L=L, Cs=Cs)
    quad_c = np.einsum("ji,ji->i", K64, np.linalg.solve(Cs @ Cs.T, K64))
    assert np.abs((cov + quad_c) - rc["cov"].astype(np.float64)).max() <= 1e-10 * (float(kxx) + quad.max())
    assert np.all(quad_c > 0) and np.all(quad_c <= quad * (1 + 1e-9))           # Cs Cs^T >= L L^T
    # variances of a conditioned GP: within [0, k**]
    assert np.all(r["cov"] > 0) and np.all(r["cov"] <= kxx)


def test_std_identity():
    """sum_q std_q^2 a_q^2 = |W^T k|^2 for W = L^-T diag(std), a = L^-1 k: W^T k = diag(std) L^-1 k.  W is formed in
    longdouble here (forward substitution on the identity), so the two sides differ by longdouble rounding only."""
    c, x, L, std, K, kxx = _problem()
    Linv = vr.forward_rows(L, np.eye(M))                        # L^-1
    W = Linv.T * std.astype(np.longdouble)[None, :]             # L^-T diag(std)
    by_std = vr.variances(K, kxx, L=L, std=std)["mcov"]
    by_w = vr.variances(K, kxx, W=W)["mcov"]
    eps_ld = np.finfo(np.longdouble).eps
    assert np.abs(by_std - by_w).max() <= 64 * M * eps_ld * np.linalg.cond(L) * by_w.max()
    # and the float64 rounding of that W gives the same to float64 accuracy (the sums W^T k cancel by up to cond(L))
    by_w64 = vr.variances(K, kxx, W=W.astype(np.float64))["mcov"]
    assert np.abs(by_std - by_w64).max() <= 64 * M * np.finfo(np.float64).eps * np.linalg.cond(L) * by_w.max()


def test_layout_and_generator():
    c, x, L, std, K, kxx = _problem()
    assert K.shape == (M, N * T) and c.shape == (M, 4) and x.shape == (N, 3)
    assert set(np.unique(c[:, -1])) <= {0.0, 1.0, 2.0, 3.0}
    # column i * T + t is query i at time t
    K1, _ = vr.product_kernel(x[2:3], TIMES[1:2], c)
    assert np.array_equal(K1[:, 0], K[:, 2 * T + 1])
    assert np.allclose(np.tril(L), L) and not L.flags.writeable
    assert abs(float(kxx) - 1.0) < 1e-5                        # Matern52 at distance sqrt(1e-12), squared
