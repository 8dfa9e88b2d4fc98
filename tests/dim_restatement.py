"""NumPy / SciPy restatement of the reference's dimensionality pieces (mellon/inference.py:95-122,142-164,195-219,
util.py:486-536, parameters.py:545-583,877-924), written from reading them.  Test infrastructure only: the product never
imports it."""
import numpy as np
from scipy.special import digamma, gammaln, polygamma

FRACTAL_SEED = 432


def ell_of(distances):
    """log of the sorted k-NN distances + log(pi) / 2 (inference.py:108-109)."""
    return np.log(np.sort(np.asarray(distances, dtype=np.float64), axis=-1)) + np.log(np.pi) / 2


def _pred(z, L, ell, mu_dim, mu_dens):
    z = np.asarray(z, dtype=np.float64).reshape(2, -1)
    D = np.exp(mu_dim + L @ z[0])
    log_dens = mu_dens + L @ z[1]
    pred = log_dens[:, None] + D[:, None] * ell - gammaln(D / 2 + 1)[:, None]
    return z, D, pred


def dim_loss(z, L, ell, mu_dim, mu_dens, K=2):
    """-(log N(z; 0, I_K-constant) + Poisson log-likelihood); the prior's constant uses K latent functions."""
    z, D, pred = _pred(z, L, ell, mu_dim, mu_dens)
    j = np.arange(1, ell.shape[1] + 1)
    lik = np.sum(pred * j - np.exp(pred) - gammaln(j))
    return 0.5 * np.sum(z ** 2) + K / 2 * np.log(2 * np.pi) - lik


def dim_grad_hess(z, L, ell, mu_dim, mu_dens):
    """Analytic gradient and Hessian diagonal, both (2, m)."""
    z, D, pred = _pred(z, L, ell, mu_dim, mu_dens)
    j = np.arange(1, ell.shape[1] + 1)
    e = np.exp(pred)
    a = j - e
    xh = D / 2 + 1
    s = ell - digamma(xh)[:, None] / 2
    tri = polygamma(1, xh)
    g1 = z[1] - L.T @ a.sum(1)
    g0 = z[0] - L.T @ (D * (a * s).sum(1))
    h1 = 1 + (L ** 2).T @ e.sum(1)
    hrow = -D * (a * s).sum(1) + D ** 2 * (e * s ** 2 + a * tri[:, None] / 4).sum(1)
    h0 = 1 + (L ** 2).T @ hrow
    return np.stack([g0, g1]), np.stack([h0, h1])


def neighbours(x, k, x_query=None):
    """The k nearest rows of x for each query (the reference's KDTree / BallTree query)."""
    from sklearn.neighbors import BallTree, KDTree
    x = np.asarray(x, dtype=np.float64)
    q = x if x_query is None else np.asarray(x_query, dtype=np.float64)
    tree = BallTree(x, metric="euclidean") if x.shape[1] >= 20 else KDTree(x, metric="euclidean")
    return tree.query(q, k=k)


def slope_lstsq(nd):
    """lstsq of log(1..kc2) on [log(sorted distances), 1]: the reference's design matrix, one neighbourhood."""
    nd = np.sort(nd)
    A = np.stack([np.log(nd), np.ones_like(nd)], axis=1)
    y = np.log(np.arange(1, nd.size + 1))
    if not np.all(np.isfinite(A)):
        return np.nan          # log 0: the reference's (JAX) lstsq returns NaN where LAPACK refuses the input
    return np.linalg.lstsq(A, y, rcond=None)[0][0]


def slope_closed(nd):
    a = np.log(np.sort(nd))
    y = np.log(np.arange(1, nd.size + 1))
    da, dy = a - a.mean(), y - y.mean()
    return np.sum(da * dy) / np.sum(da * da)


def slope_rank_rule(nd):
    """The device's rule (k_local_dim), restated: lstsq's rank test on A = [a, 1] from the 2 x 2 normal matrix
    (s_min <= eps max(kc2, 2) s_max  <=>  det(A^T A) <= (eps max(kc2, 2) lam1)^2, det = kc2 Sxx), then the closed-form slope
    at full rank or the minimum-norm solution v1 v1^T A^T y / lam1 at rank 1."""
    a = np.log(np.sort(nd))
    y = np.log(np.arange(1, nd.size + 1))
    if not np.all(np.isfinite(a)):
        return np.nan
    N = float(a.size)
    abar, ybar = a.mean(), y.mean()
    da, dy = a - abar, y - ybar
    sxx, sxy = np.sum(da * da), np.sum(da * dy)
    p, q = sxx + N * abar * abar, N * abar
    h = 0.5 * (p - N)
    disc = np.hypot(h, q)
    lam1 = 0.5 * (p + N) + disc
    tol = np.finfo(np.float64).eps * max(N, 2.0) * lam1
    if N * sxx > tol * tol:
        return sxy / sxx
    v = np.array([disc + h, q]) if h >= 0 else np.array([q, disc - h])
    aty = np.array([sxy + N * abar * ybar, N * ybar])
    return v[0] * (v @ aty) / ((v @ v) * lam1)


def one_hot_rows(k):
    """k rows of the identity: every pair distance is exactly sqrt(2)."""
    return np.eye(k)


def rotated_simplex(k, seed):
    """The rows Q e_i of a random orthogonal Q (k x k): pair distances sqrt(2) up to rounding."""
    Q = np.linalg.qr(np.random.default_rng(seed).normal(size=(k, k)))[0]
    return np.ascontiguousarray(Q.T)


def pair_distances(nb):
    """The k(k-1)/2 distances among the rows of one neighbourhood (k x d)."""
    i, j = np.triu_indices(nb.shape[0], k=1)
    return np.linalg.norm(nb[i] - nb[j], axis=-1)


def local_dimensionality(x, k=30, x_query=None, neighbor_idx=None):
    x = np.asarray(x, dtype=np.float64)
    k = min(k, x.shape[0])
    if neighbor_idx is None:
        neighbor_idx = neighbours(x, k, x_query)[1]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.array([slope_lstsq(pair_distances(x[idx])) for idx in np.asarray(neighbor_idx)])


def ridge(L, target):
    """sklearn Ridge(alpha=1, fit_intercept=False).coef_ in closed form."""
    m = L.shape[1]
    return np.linalg.solve(L.T @ L + np.eye(m), L.T @ target)


def mle(nn, d):
    return gammaln(d / 2 + 1) - (d / 2) * np.log(np.pi) - d * np.log(nn)


def initial_dimensionalities(L, d, mu_dim, nn, mu_dens):
    target = np.log(d) - mu_dim
    if np.size(target) == 1:
        target = np.full(L.shape[0], float(target))
    return np.stack([ridge(L, target), ridge(L, mle(nn, d) - mu_dens)])


def fractal_d(x, k=10, n=500, seed=FRACTAL_SEED):
    """compute_d_factal with the mirror's documented draw (NumPy, not JAX)."""
    x = np.asarray(x, dtype=np.float64)
    if n < x.shape[0]:
        q = x[np.random.default_rng(seed).choice(x.shape[0], size=n, replace=False)]
    else:
        q = x
    return float(np.mean(local_dimensionality(x, k=k, x_query=q)))
