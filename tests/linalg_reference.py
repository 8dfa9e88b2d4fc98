"""The yardstick of the Cholesky and triangular-solve tests: residuals and substitutions in np.longdouble (64-bit
significand on x86: 2^-11 of a double's rounding unit), the crafted matrices the device is asked to factor, the two bounds
the device is held to, and a plain-NumPy emulation of the device's blocked algorithms in float64 building blocks.
tests/test_linalg_reference_host.py checks all of it on the CPU (and that the bounds are reachable by the design);
tests/test_gpu_linalg.py measures the device and LAPACK against it.  The product never imports this file."""
import functools

import numpy as np
import scipy.linalg as sla

EPS = 2.0 ** -52
NB = 128                # block width of the device's factorisation and of its explicitly inverted diagonal blocks


# ---- residuals and references in longdouble ---------------------------------------------------------------------------
def chol_backward(L, A):
    """max |L L^T - A| / max |A| over the lower triangle, in longdouble (the strict upper triangle of A is never read)."""
    Ll = np.tril(np.asarray(L, dtype=np.float64)).astype(np.longdouble)
    Al = np.tril(np.asarray(A, dtype=np.float64)).astype(np.longdouble)
    worst = np.longdouble(0.0)
    for i0 in range(0, Ll.shape[0], NB):          # block rows: columns past the block's last row are zero in L
        i1 = min(i0 + NB, Ll.shape[0])
        R = np.tril(Ll[i0:i1, :i1] @ Ll[:i1, :i1].T, i0) - Al[i0:i1, :i1]
        worst = max(worst, np.abs(R).max())
    return float(worst / np.abs(Al).max())


def solve_lower_longdouble(Lf, B, trans=False):
    """Lf^-1 B (trans: Lf^-T B) by row-by-row substitution in longdouble, all columns of B at once; only the lower
    triangle of Lf is read."""
    T = np.tril(np.asarray(Lf, dtype=np.float64)).astype(np.longdouble)
    X = np.array(B, dtype=np.longdouble)
    one_d = X.ndim == 1
    X = X.reshape(T.shape[0], -1)
    m = T.shape[0]
    if not trans:
        for i in range(m):
            X[i] = (X[i] - T[i, :i] @ X[:i]) / T[i, i]
    else:
        for i in range(m - 1, -1, -1):
            X[i] = (X[i] - T[i + 1:, i] @ X[i + 1:]) / T[i, i]
    return X[:, 0] if one_d else X


def forward_error(X, Xref):
    """max |X - Xref| / max |Xref|, the difference taken in longdouble."""
    Xr = np.asarray(Xref, dtype=np.longdouble)
    return float(np.abs(np.asarray(X, dtype=np.float64).astype(np.longdouble) - Xr).max() / np.abs(Xr).max())


def skeel_blocks(Lref, nb=NB):
    """S_blk = max_j || |T_jj^-1| |T_jj| ||_inf over the nb-wide diagonal blocks T_jj of a reference factor: what an
    explicitly inverted diagonal block costs over a substitution (the inverses are taken in longdouble)."""
    Lref = np.asarray(Lref, dtype=np.float64)
    m = Lref.shape[0]
    worst = 0.0
    for j0 in range(0, m, nb):
        T = np.tril(Lref[j0:j0 + nb, j0:j0 + nb])
        Ti = np.asarray(solve_lower_longdouble(T, np.eye(T.shape[0])), dtype=np.longdouble)
        worst = max(worst, float((np.abs(Ti) @ np.abs(T).astype(np.longdouble)).sum(axis=1).max()))
    return worst


def chol_bound(e_lap, s_blk):
    """4 e_lap + EPS S_blk.  4 e_lap: the margin slogdet_reference.py gives another summation order over LAPACK's own
    error.  EPS S_blk: the panel is A21 fl(T^-1)^T, not a substitution; its residual A21 (I - X T^T) is bounded to first
    order by gamma_128 || |T^-1| |T| || ||A21|| -- with the factor 128 of gamma_128 deliberately dropped, because the
    worst case is never approached (the emulation below sits 16 to 50 times under the bound) and a bound 128 times wider
    would pass a kernel that loses two more digits."""
    return 4.0 * e_lap + EPS * s_blk


def solve_bound(f_lap, m):
    """4 f_lap + m EPS: LAPACK's own forward error with the same margin, plus the floor of an m-term dot product
    relative to the largest entry."""
    return 4.0 * f_lap + m * EPS


# ---- crafted inputs (all seeded) --------------------------------------------------------------------------------------
def kernel_like(m, seed, jitter=1e-6):
    """The exp-quad matrix of m Gaussian points in 4-D plus jitter I (as _kernel_like of tests/test_gpu_ops.py): the
    workload's K_uu + jitter I, cond(A) ~ 1e8 and cond(L) ~ 1e4 at the default jitter."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(m, 4))
    xx = (x * x).sum(1)
    d2 = np.maximum(xx[:, None] - 2 * x @ x.T + xx[None, :], 0.0)
    return np.exp(-0.5 * d2 / 4.0) + jitter * np.eye(m)


def benign(m, seed):
    """B B^T / m + 0.1 I, the matrix test_cholesky of tests/test_gpu_ops.py uses."""
    rng = np.random.default_rng(seed)
    B = rng.normal(size=(m, m + 3))
    return B @ B.T / m + np.eye(m) * 0.1


def benign_factor(m, seed):
    """0.1 tril(N) + 2 I, the factor test_trsm of tests/test_gpu_ops.py uses (condition number 6 to 16)."""
    rng = np.random.default_rng(seed)
    return np.tril(rng.normal(size=(m, m))) * 0.1 + np.eye(m) * 2.0


def graded(A, seed):
    """(D A D, d) with d = 2^k, k uniform integers in [-20, 20]: an exact scaling, so chol(D A D) = D chol(A) in exact
    arithmetic and every product d_i a_ij d_j is exact in float64."""
    rng = np.random.default_rng(seed)
    d = 2.0 ** rng.integers(-20, 21, size=A.shape[0])
    return A * d[:, None] * d[None, :], d


def bad_pivot(A, k, kind):
    """A copy of the positive definite A whose first failing pivot is k in ANY Cholesky: with L = chol(A), A[k, k] becomes
    sum_{j<k} L[k, j]^2 - 0.5 ("negative": pivot k is about -0.5) or NaN ("nan").  The leading k x k block is untouched,
    so pivots 0 .. k-1 stay positive."""
    L = sla.cholesky(A, lower=True)
    out = np.array(A, dtype=np.float64)
    if kind == "negative":
        out[k, k] = float(L[k, :k] @ L[k, :k]) - 0.5
    elif kind == "nan":
        out[k, k] = np.nan
    else:
        raise ValueError(kind)
    return out


# ---- the device's algorithms in plain NumPy (float64 building blocks) --------------------------------------------------
def _inv_lower_by_substitution(T):
    """T^-1 of a lower-triangular block, column by column by forward substitution (float64)."""
    n = T.shape[0]
    X = np.zeros((n, n))
    for i in range(n):
        e = np.zeros(n)
        e[i] = 1.0
        X[i] = (e - T[i, :i] @ X[:i]) / T[i, i]
    return X


def _chol_unblocked(A):
    """Unblocked lower Cholesky of a small block (float64, left-looking by columns); None at a non-positive pivot."""
    n = A.shape[0]
    L = np.zeros((n, n))
    for k in range(n):
        d = A[k, k] - L[k, :k] @ L[k, :k]
        if not d > 0.0:
            return None
        L[k, k] = np.sqrt(d)
        L[k + 1:, k] = (A[k + 1:, k] - L[k + 1:, :k] @ L[k, :k]) / L[k, k]
    return L


def first_bad_pivot(A):
    """Index of the first pivot that is not positive (non-positive or NaN: the test of LAPACK's dpotf2), -1 if none:
    unblocked Cholesky in float64 on the lower triangle."""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    L = np.zeros((n, n))
    for k in range(n):
        d = A[k, k] - L[k, :k] @ L[k, :k]
        if not d > 0.0:
            return k
        L[k, k] = np.sqrt(d)
        L[k + 1:, k] = (A[k + 1:, k] - L[k + 1:, :k] @ L[k, :k]) / L[k, k]
    return -1


def emulate_cholesky(A, nb=NB):
    """The blocked factorisation as the device runs it: each nb-wide diagonal block is factored, its inverse X formed by
    substitution, the panel is A21 X^T (a product with the explicit inverse, NOT a substitution), then the trailing
    update A22 -= P P^T."""
    W = np.tril(np.array(A, dtype=np.float64))
    W = W + np.tril(W, -1).T
    m = W.shape[0]
    L = np.zeros((m, m))
    for j0 in range(0, m, nb):
        j1 = min(j0 + nb, m)
        T = _chol_unblocked(W[j0:j1, j0:j1])
        if T is None:
            raise np.linalg.LinAlgError("not positive definite")
        L[j0:j1, j0:j1] = T
        if j1 == m:
            break
        P = W[j1:, j0:j1] @ _inv_lower_by_substitution(T).T
        L[j1:, j0:j1] = P
        W[j1:, j1:] -= P @ P.T
    return L


def block_scaled_copies(Lf, nb=NB):
    """(W, W2) of a lower factor as the device builds them: W[j, <=j] = Dinv_j [-Lf[j, <j] | I] (row-scaled) and
    W2[>=j, j] = [I ; -Lf[>j, j]] Dinv_j (column-scaled), Dinv_j the explicit inverse of the diagonal block."""
    Lf = np.tril(np.asarray(Lf, dtype=np.float64))
    m = Lf.shape[0]
    W, W2 = np.zeros((m, m)), np.zeros((m, m))
    for j0 in range(0, m, nb):
        j1 = min(j0 + nb, m)
        D = _inv_lower_by_substitution(Lf[j0:j1, j0:j1])
        W[j0:j1, j0:j1] = D
        W2[j0:j1, j0:j1] = D
        W[j0:j1, :j0] = -(D @ Lf[j0:j1, :j0])
        W2[j1:, j0:j1] = -(Lf[j1:, j0:j1] @ D)
    return W, W2


def emulate_solve(copies, B, trans, right_looking, nb=NB):
    """Lf^-1 B (trans: Lf^-T B) from copies = block_scaled_copies(Lf, nb) by the device's two routes.  Left-looking: one product per block row against the scaled
    copy.  Right-looking: updates of the un-multiplied block rows B~ against the other copy, then ONE block-diagonal
    product X_j = Dinv_j B~_j (trans: Dinv_j^T B~_j)."""
    W, W2 = copies
    X = np.array(B, dtype=np.float64).reshape(W.shape[0], -1)
    m = X.shape[0]
    starts = list(range(0, m, nb))
    if not right_looking:
        if not trans:
            for j0 in starts:
                j1 = min(j0 + nb, m)
                X[j0:j1] = W[j0:j1, :j1] @ X[:j1]
        else:
            for j0 in reversed(starts):
                j1 = min(j0 + nb, m)
                X[j0:j1] = W2[j0:, j0:j1].T @ X[j0:]
        return X
    if not trans:
        for j0 in starts:
            j1 = min(j0 + nb, m)
            if j1 < m:
                X[j1:] += W2[j1:, j0:j1] @ X[j0:j1]
    else:
        for j0 in reversed(starts[1:]):
            j1 = min(j0 + nb, m)
            X[:j0] += W[j0:j1, :j0].T @ X[j0:j1]
    for j0 in starts:
        j1 = min(j0 + nb, m)
        D = W[j0:j1, j0:j1]
        X[j0:j1] = (D.T if trans else D) @ X[j0:j1]
    return X


def emulate_solve_right_T(copies, Xin, right_looking, nb=NB):
    """X Lf^-T from copies = block_scaled_copies(Lf, nb) by the device's two routes: left-looking X_j <- [X_<j | X_j] W_j^T over block columns, or right-looking
    X_>j += X~_j W2[>j, j]^T with one block-diagonal product X = X~ blockdiag(Dinv^T) at the end."""
    W, W2 = copies
    X = np.array(Xin, dtype=np.float64)
    m = W.shape[0]
    if not right_looking:
        for j0 in range(0, m, nb):
            j1 = min(j0 + nb, m)
            X[:, j0:j1] = X[:, :j1] @ W[j0:j1, :j1].T
        return X
    for j0 in range(0, m, nb):
        j1 = min(j0 + nb, m)
        if j1 < m:
            X[:, j1:] += X[:, j0:j1] @ W2[j1:, j0:j1].T
    for j0 in range(0, m, nb):
        j1 = min(j0 + nb, m)
        X[:, j0:j1] = X[:, j0:j1] @ W[j0:j1, j0:j1].T
    return X


# ---- the cases of tests/test_gpu_linalg.py, named once so that the host test can vouch for them ------------------------
CHOL_SIZES = (16, 17, 127, 128, 129, 255, 256, 257, 384, 385, 513)
CHOL_BENIGN_SIZES = (129, 385)
BAD_PIVOT_M = 385
BAD_PIVOT_KS = (0, 15, 16, 127, 128, 129, 255, 256, 300, 384)
BAD_PIVOT_KINDS = ("negative", "nan")
TRSM_SIZES = (1, 63, 64, 65, 127, 128, 129, 193, 256, 257, 385)
TRSM_RHS = (1, 2, 255, 256, 257)
TRSM_BENIGN_SIZES = (129, 385)


def seed_of(family, m):
    """One seed per (family, m), shared by the host test and the GPU test."""
    return {"kernel_like": 1000, "benign": 2000, "benign_factor": 3000}[family] + m


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def make_matrix(family, m):
    return {"kernel_like": kernel_like, "benign": benign}[family](m, seed_of(family, m))


@functools.lru_cache(maxsize=None)
def chol_case(family, m, add_diag=0.0):
    """(A, e_lap, S_blk) of one factorisation case, computed once and read-only: the input A (add_diag NOT yet added),
    LAPACK's backward error on A + add_diag I and the block Skeel number of LAPACK's factor."""
    A = make_matrix(family, m)
    Afull = A + add_diag * np.eye(m)
    Lref = sla.cholesky(Afull, lower=True)
    _frozen(A)
    return A, chol_backward(Lref, Afull), skeel_blocks(Lref)


@functools.lru_cache(maxsize=None)
def trsm_case(family, m, trans):
    """(Lf, B, Xref) of one solve case, computed once and read-only: B is m x max(TRSM_RHS) standard normal and Xref the
    longdouble solution; the columns of a solve are independent, so a case with p right-hand sides uses B[:, :p] and
    Xref[:, :p]."""
    if family == "kernel_like":
        Lf = sla.cholesky(kernel_like(m, seed_of(family, m)), lower=True)
    else:
        Lf = benign_factor(m, seed_of(family, m))
    B = np.random.default_rng(seed_of(family, m) + 7).normal(size=(m, max(TRSM_RHS)))
    return _frozen(Lf, B, solve_lower_longdouble(Lf, B, trans))


def lapack_solve(Lf, B, trans):
    return sla.solve_triangular(Lf, B, lower=True, trans="T" if trans else "N")
