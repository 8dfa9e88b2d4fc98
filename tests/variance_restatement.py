"""Extended-precision restatement of the three predictive variances of a time-sensitive predictor at (query, time) pairs
(reference conditional.py:409-440, 707-716), with the kernel formulas of predict_restatement, and the generator of the
variance-grid tests.  For the kernel column k = cov(centres, (x, t)) (m values) and k** = cov((x, t), (x, t)):
    covariance       k** - |a|^2,           a = L^-1 k  by row-by-row forward substitution
                     (+ |Cs^-1 k|^2 for the noisy landmark conditional: k** - (k** - |Cs^-1 k|^2) added)
    mean covariance  |W^T k|^2              W (m x q), or  sum_q std_q^2 a_q^2  for W = L^-T diag(std)
    uncertainty      their sum
Everything is np.longdouble; the float64 inputs (L, Cs, W, std) are taken as exact.  Also returned: the magnitudes
S_cov = k** + |a|^2 and S_mcov = |W^T k|^2 that the tests' error measure divides by.  Test infrastructure only: the product
never imports it."""
import numpy as np

import predict_restatement as pr

LD = np.longdouble
LS_STATE, LS_TIME = 2.6, 1.3


def product_kernel(x, times, c, kind="Matern52", ls_state=LS_STATE, ls_time=LS_TIME):
    """(K, kxx) in longdouble for cov = kind(ls_state) on the state columns x kind(ls_time) on the last column:
    K[j, i * T + t] = cov(c_j, (x_i, times_t)) (m, n T) -- column order of a row-major (n, T) result -- and kxx =
    cov(z, z), one number for a stationary product."""
    x, c = np.asarray(x, dtype=np.float64), np.asarray(c, dtype=np.float64)
    times = np.asarray(times, dtype=np.float64).reshape(-1, 1)
    Ks, _ = pr.kernel_ref(kind, ls_state, c[:, :-1], x[:, :c.shape[1] - 1])          # (m, n)
    Kt, _ = pr.kernel_ref(kind, ls_time, c[:, -1:], times)                            # (m, T)
    K = (Ks[:, :, None] * Kt[:, None, :]).reshape(c.shape[0], -1)
    z = np.zeros((1, 1))
    kxx = pr.kernel_ref(kind, ls_state, z, z)[0][0, 0] * pr.kernel_ref(kind, ls_time, z, z)[0][0, 0]
    return K, kxx


def forward_rows(L, B):
    """L^-1 B for lower-triangular L (m x m) and B (m x N), row by row, in longdouble."""
    L, B = np.asarray(L).astype(LD), np.asarray(B).astype(LD)
    A = np.zeros_like(B)
    for j in range(L.shape[0]):
        A[j] = (B[j] - L[j, :j] @ A[:j]) / L[j, j]
    return A


def variances(K, kxx, L=None, Cs=None, W=None, std=None):
    """dict of longdouble vectors over the columns of K: cov, S_cov (with L), mcov, S_mcov (with W, or std and L)."""
    out = {}
    K = np.asarray(K).astype(LD)
    if L is not None:
        A = forward_rows(L, K)
        a2 = np.square(A).sum(axis=0)
        out["cov"] = LD(kxx) - a2
        out["S_cov"] = LD(kxx) + a2
        if Cs is not None:
            b2 = np.square(forward_rows(Cs, K)).sum(axis=0)
            out["cov"] = out["cov"] + (LD(kxx) - (LD(kxx) - b2))
        if std is not None:
            out["mcov"] = (np.square(np.asarray(std).astype(LD))[:, None] * np.square(A)).sum(axis=0)
    if W is not None:
        assert std is None
        out["mcov"] = np.square(np.asarray(W).astype(LD).T @ K).sum(axis=0)
    if "mcov" in out:
        out["S_mcov"] = out["mcov"]
    return out


def make_problem(n, m, seed, d_state=3):
    """The generator of the CPU trial: centres and queries 1.5 N(0, 1) in d_state columns, centre times in {0, 1, 2, 3},
    L = chol(K_uu + 1e-6 I) in float64 (cond(L) ~ 1.6e2 at m = 130), std in [0.05, 0.5].  Returns (c, x, L, std), read-only."""
    rng = np.random.default_rng(seed)
    c = np.concatenate([rng.normal(size=(m, d_state)) * 1.5, rng.integers(0, 4, size=(m, 1)).astype(np.float64)], axis=1)
    x = rng.normal(size=(n, d_state)) * 1.5
    Ks, _ = pr.kernel_ref("Matern52", LS_STATE, c[:, :-1], c[:, :-1])
    Kt, _ = pr.kernel_ref("Matern52", LS_TIME, c[:, -1:], c[:, -1:])
    Kuu = (Ks * Kt).astype(np.float64)
    L = np.linalg.cholesky(Kuu + 1e-6 * np.eye(m))
    std = rng.uniform(0.05, 0.5, size=m)
    for a in (c, x, L, std):
        a.flags.writeable = False
    return c, x, L, std
