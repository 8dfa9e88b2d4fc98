"""The yardstick of the objective-pass tests (csrc/objective.hip): the quantities of one evaluation in np.longdouble
(64-bit significand on x86), forward-error bounds that hold for ANY summation order, the dispatch of launch_objective
restated, and the case lists.  tests/test_objective_reference_host.py checks all of it on the CPU (the reference against
exact rationals, the bounds against a float64 evaluation, and that every mutation a wrong guard would amount to moves a
checked quantity far beyond its bound); tests/test_gpu_objective.py holds the device to it.  The product never imports
this file.

Quantities (include/mellon_hip.h at mln_objective; the row-list comment of objective.hip), for L (n x m), V, Vdr, mu, z,
an optional row list and weights w (1 without):
    f = L z + mu,  t = f + V,  e = exp(t),  a = w e,
    lik = sum_i (a_i - (f_i + Vdr_i)),  g = L^T (a - 1),  h = (L o L)^T e,
and with the prior terms of mln_objective: loss = lik + 1/2 |z|^2 + (m / 2) log 2 pi, grad = g + z, hess = h + 1.

Bounds, with u = 2^-53 and gamma_k = k u / (1 - k u):
    df_i   = gamma_40 (sum_j |L_ij z_j| + |mu|)      40: at most 16 fused steps per thread, 6 shuffle levels, 8 wave
                                                     partials, + mu, up to 8 segment accumulations, and slack
    dt_i   = df_i + u |t_i|
    da_i   = a_i (1.01 dt_i + 4 u)                   4 u: the device exp and the product with w
    dlik   = sum_i (da_i + df_i) + gamma_{n+3} sum_i (|a_i| + |f_i| + |Vdr_i|)
    dg_j   = sum_i |L_ij| da_i + gamma_{n+2} sum_i |L_ij| |a_i - 1|
    dh_j   = sum_i L_ij^2 da_i + gamma_{n+3} sum_i L_ij^2 e_i
    prior: + gamma_{m+2} 1/2 |z|^2,  + u |z_j|,  + u
           and on the loss + 5 u (|lik| + 1/2 |z|^2 + (m / 2) log 2 pi): the constant is a rounded product of a rounded
           logarithm of a rounded 2 pi (3 u of it), and the two final additions round once each (u |lik + 1/2 |z|^2| and
           u |loss|).  Without this term no double can meet the bound at z = 0, n = 1, m = 1024: there the bound is
           1.4e-14 and half an ulp of the loss (944) is 5.7e-14 -- the nearest double to the exact loss would fail.
A device result passes when |got - ref| <= 2 x bound, element by element (the 2 covers the first-order terms dropped).
The bounds themselves are sums of non-negative terms and are evaluated in float64: their own rounding (a relative
gamma_n) disappears in that factor.

Where np.longdouble is only a double (nmant < 63) every sum goes through math.fsum over error-free products instead
(`exact=True`, tested here on every machine), the reference values are then correctly rounded doubles, and half an ulp of
each is added to its bound -- never a silent comparison of double against double.
"""
import math
import types

import numpy as np

LD = np.longdouble
EXTENDED = np.finfo(LD).nmant >= 63
U = 2.0 ** -53
WG = 512
SEG = 8192
N_CU = 256                      # compute units of an MI355X: the workgroup count the row split is stated for
LOG_2PI = np.log(LD(8.0) * np.arctan(LD(1.0)))


def gamma(k):
    return k * U / (1.0 - k * U)


def pad16(m):
    return (m + 15) // 16 * 16


# ---- dispatch of launch_objective / launch_objective_wide, restated ----------------------------------------------------
MODES = ("obj", "hess", "gemvt", "fonly")
# cpt -> (CPT, R, VEC) of MODE_OBJ / MODE_OBJ_HESS, and of MODE_GEMVT / MODE_FONLY
_FUSED = {1: (1, 8, True), 2: (2, 8, True), 3: (3, 4, True), 4: (4, 2, False), 5: (5, 2, False), 6: (6, 2, False),
          7: (8, 1, False), 8: (8, 1, False)}
_PLAIN = {1: (1, 8, False), 2: (2, 5, False), 3: (3, 3, False), 4: (4, 2, False), 5: (5, 2, False), 6: (6, 2, False),
          7: (8, 1, False), 8: (8, 1, False)}


def cpt_of(m, segment=False):
    """Column pairs per thread: of a whole matrix with m <= 8192 columns (pairs = pad16(m) / 2), or of a column segment
    of a wider one (pairs = (seg_cols + 1) / 2)."""
    assert 1 <= m <= SEG
    pairs = (m + 1) // 2 if segment else pad16(m) // 2
    return (pairs + WG - 1) // WG


def variant(m, mode, segment=False):
    """(CPT, R, VEC) of the k_objective instantiation launch_objective picks."""
    assert mode in MODES
    return (_FUSED if mode in ("obj", "hess") else _PLAIN)[cpt_of(m, segment)]


def segments(m):
    """[(c0, seg_cols, lim, store_lim)] of launch_objective_wide; a matrix of at most 8192 columns has none (one launch).
    lim: column pairs a lane may read from the segment's pointer; store_lim: columns of the partial buffer it writes."""
    if m <= SEG:
        return []
    ldl = pad16(m)
    return [(c0, min(SEG, m - c0), (ldl - c0) // 2, (min(SEG, m - c0) + 1) & ~1) for c0 in range(0, m, SEG)]


def launches(m, call):
    """The instantiations one API call runs: call in 'objective', 'objective_hess', 'transform', 'gemvt', 'rows'."""
    if m <= SEG:
        mode = {"objective": "obj", "objective_hess": "hess", "transform": "fonly", "gemvt": "gemvt", "rows": "obj"}[call]
        return [variant(m, mode)]
    if call in ("objective_hess", "rows"):
        return None                                     # MLN_ERR_UNSUPPORTED
    segs = segments(m)
    out = []
    if call in ("objective", "transform"):
        out += [variant(s[1], "fonly", True) for s in segs]
    if call in ("objective", "gemvt"):
        out += [variant(s[1], "gemvt", True) for s in segs]
    return out


def row_split(n, R, n_wg=None, n_cu=N_CU):
    """(n_wg, steps of each workgroup) of a pass over n rows in steps of R (k_objective's contiguous ranges)."""
    if n_wg is None:
        n_wg = max(1, min(n_cu, (n + 1) // 2))
    nsteps = (n + R - 1) // R
    per = (nsteps + n_wg - 1) // n_wg
    return n_wg, [max(0, min(nsteps, (w + 1) * per) - w * per) for w in range(n_wg)]


# ---- case lists ----------------------------------------------------------------------------------------------------------
M_EDGES = [1, 2, 3, 16, 17, 1024, 1025, 2048, 2049, 3072, 3073, 4096, 4097, 5120, 5121, 6144, 6145, 7168, 7169, 8191, 8192,
           8193,        # second segment: one column, lim = 8
           8194,
           9217,        # second segment needs CPT = 2
           16384,
           16385]       # three segments
N_EDGES = [1, 9, 10, 533, 2057]
N_EXACT = 16            # one more row count: an exact last step for R = 8 and 4 (none of N_EDGES is a multiple of 4)
M_LOWER = [1, 1025, 2049, 3073, 4097, 5121, 6145, 7169, 8193]      # where n = 2057 is taken: the first m of every cpt
VALUE_CASES = [(n, m) for m in M_EDGES for n in N_EDGES + [N_EXACT] if n != 2057 or m in M_LOWER]

RIDGE_N = 533
RIDGE_M = [1025, 2049, 3073, 4097, 5121, 6145, 7169, 8192, 8193]

ROWS_N = 1000
ROWS_M = [300, 1500, 2100, 3210, 4100, 5200, 6200, 8192]
ROWS_COUNTS = [1, 7, 8, 9, 17, 255, 257, 700, 1000]

OVERFLOW_N = 10
OVERFLOW_M = [300, 4100, 8193]


def progressions(count, n=ROWS_N):
    """(first, stride) of the strided launches over `count` of n rows: the leading rows, one that ends on the last row,
    one in between."""
    last = (n - 1, 1) if count == 1 else ((n - 1) - (count - 1) * ((n - 1) // (count - 1)), (n - 1) // (count - 1))
    mid = (3, max(1, (n - 8) // count))
    out = []
    for first, stride in ((0, 1), last, mid):
        if first + (count - 1) * stride < n and (first, stride) not in out:
            out.append((first, stride))
    assert last in out
    return out


def case_seed(n, m):
    return 100_003 * n + m


def make_problem(n, m, seed):
    """L ~ N(0, (0.5 / sqrt m)^2); z ~ 0.3 N(0, 1) with weight on the last two real columns (a wrong `col + 1 < m` guard
    then moves f by far more than its bound); V, Vdr ~ N(0, 1) independently (a swap shows); the last row dominates."""
    rng = np.random.default_rng(seed)
    L = rng.normal(size=(n, m)) * (0.5 / np.sqrt(m))
    z = 0.3 * rng.normal(size=m)
    z[m - 1] = 2.0
    if m >= 2:
        z[m - 2] = -1.5
    V = rng.normal(size=n)
    Vdr = rng.normal(size=n)
    V[n - 1] += 2.0
    return L, V, Vdr, -3.0, z


# ---- sums: long double, or error-free products through math.fsum -----------------------------------------------------
def _two_prod(a, b):
    """p + e == a b exactly (Dekker), element-wise on float64 arrays of moderate magnitude."""
    p = a * b

    def split(x):
        c = 134217729.0 * x
        hi = c - (c - x)
        return hi, x - hi

    ah, al = split(a)
    bh, bl = split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _fsum_products(pairs):
    """Correctly rounded sum_k a_k b_k over all the (a, b) vector pairs."""
    terms = []
    for a, b in pairs:
        p, e = _two_prod(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
        terms += p.tolist() + e.tolist()
    return math.fsum(terms)


def _matvec(A, x, exact, Aq=None):
    """A x: rows in long double (Aq: A already widened), or (exact) each row's correctly rounded double."""
    if not exact:
        return (A.astype(LD) if Aq is None else Aq) @ np.asarray(x).astype(LD)
    return np.array([_fsum_products([(A[i], x)]) for i in range(A.shape[0])], dtype=np.float64).astype(LD)


def reference_f(L, z, mu, rows=None, exact=not EXTENDED, Lq=None):
    """(f, df): f = L z + mu of the rows and its bound."""
    Lr = L if rows is None else L[np.asarray(rows)]
    z = np.asarray(z, dtype=np.float64)
    f = _matvec(Lr, z, exact, Lq) + LD(mu)
    df = gamma(40) * (np.abs(Lr) @ np.abs(z) + abs(mu))
    if exact:
        df = df + 2.0 * U * np.abs(f).astype(np.float64)      # the rounded row sums, and their sum with mu
    return f, df


def lik_and_bound(f, df, V, Vdr, w=None, exact=not EXTENDED):
    """(lik, dlik, t, e, a, da) from the rows' f and its bound: the row-wise part of the evaluation."""
    n = f.shape[0]
    t = f + V.astype(LD)
    e = np.exp(t)                                             # (exact: a double exp, one more u in da)
    a = e if w is None else np.asarray(w).astype(LD) * e
    a64 = a.astype(np.float64)
    dt = df + U * np.abs(t).astype(np.float64)
    da = a64 * (1.01 * dt + (6.0 if exact else 4.0) * U)
    terms = a - (f + Vdr.astype(LD))
    lik = LD(math.fsum(terms.astype(np.float64).tolist())) if exact else terms.sum()
    mag = (np.abs(a64) + np.abs(f).astype(np.float64) + np.abs(Vdr)).sum()
    dlik = (da + df).sum() + gamma(n + 3) * mag
    if exact:
        dlik += 3.0 * U * mag
    return lik, float(dlik), t, e, a, da


def reference(L, V, Vdr, mu, z, rows=None, w=None, hess=True, prior=True, exact=not EXTENDED):
    """One evaluation and its bounds.  rows / w: the row list and its weights (V, Vdr indexed by the listed row, w by the
    position in the list); prior=False: what one launch and its reduction leave (mln_diag_objective_rows)."""
    Lr = L if rows is None else L[np.asarray(rows)]
    Vr = V if rows is None else V[np.asarray(rows)]
    Vdrr = Vdr if rows is None else Vdr[np.asarray(rows)]
    z = np.asarray(z, dtype=np.float64)
    n, m = Lr.shape
    Lq = None if exact else Lr.astype(LD)
    f, df = reference_f(Lr, z, mu, exact=exact, Lq=Lq)
    lik, dlik, t, e, a, da = lik_and_bound(f, df, Vr, Vdrr, w, exact)
    coef = a - LD(1.0)
    A = np.abs(Lr)
    dg = da @ A + gamma(n + 2) * (np.abs(coef).astype(np.float64) @ A)
    if exact:
        c64 = coef.astype(np.float64)
        clo = (coef - c64.astype(LD)).astype(np.float64)
        g = np.array([_fsum_products([(Lr[:, j], c64), (Lr[:, j], clo)]) for j in range(m)], dtype=np.float64).astype(LD)
        dg = dg + U * np.abs(g).astype(np.float64)
    else:
        g = coef @ Lq
    out = types.SimpleNamespace(f=f, df=df, t=t, e=e, a=a, da=da, lik=lik, dlik=dlik)
    if hess:
        L2 = Lr * Lr
        dh = da @ L2 + gamma(n + 3) * (e.astype(np.float64) @ L2)
        if exact:
            sq, sqe = _two_prod(Lr, Lr)
            e64 = e.astype(np.float64)
            h = np.array([_fsum_products([(sq[:, j], e64), (sqe[:, j], e64)]) for j in range(m)], dtype=np.float64).astype(LD)
            dh = dh + U * np.abs(h).astype(np.float64)
        else:
            h = np.einsum("i,ij,ij->j", e, Lq, Lq)
    if prior:
        zq = z.astype(LD)
        half = LD(0.5) * (zq @ zq)
        const = LD(m) / 2 * LOG_2PI
        out.loss = lik + half + const
        out.dloss = dlik + gamma(m + 2) * float(half) + 5.0 * U * (abs(float(lik)) + float(half) + float(const)) \
            + (U * abs(float(out.loss)) if exact else 0.0)
        out.grad, out.dgrad = g + zq, dg + U * np.abs(z)
        if hess:
            out.hess, out.dhess = h + LD(1.0), dh + U
    else:
        out.loss, out.dloss, out.grad, out.dgrad = lik, dlik, g, dg
        if hess:
            out.hess, out.dhess = h, dh
    return out


def scaled(value, bound, s):
    """Reference and bound of a result the kernel multiplied by out_scale (one more rounding)."""
    return value * LD(s), bound * s + U * np.abs(np.asarray(value * LD(s), dtype=np.float64))


def ratio(got, ref, bound):
    """Worst |got - ref| / bound over the elements; a non-finite result counts as infinitely far."""
    got = np.atleast_1d(np.asarray(got, dtype=np.float64))
    if not np.isfinite(got).all():
        return math.inf
    d = np.abs(got.astype(LD) - np.atleast_1d(ref))
    return float(np.max(d / np.atleast_1d(bound)))


def evaluate64(L, V, Vdr, mu, z, w=None):
    """The same evaluation in plain float64 NumPy: loss, grad, hess, f with the prior terms (what the bounds must admit)."""
    f = L @ z + mu
    e = np.exp(f + V)
    a = e if w is None else w * e
    loss = (a - (f + Vdr)).sum() + 0.5 * (z @ z) + 0.5 * L.shape[1] * math.log(2.0 * math.pi)
    return loss, (a - 1.0) @ L + z, e @ (L * L) + 1.0, f


# ---- the Ridge start: z0 = L^T (L L^T + I)^-1 t -----------------------------------------------------------------------
def ridge_reference(L, t, chunk=512):
    """Woodbury form of (L^T L + I)^-1 L^T t: an n x n system (condition < 3 with make_problem's scaling), solved by a
    long-double Cholesky; the products with L^T in long double.  The Gram matrix L L^T is accumulated in long double over
    float64 products of `chunk` columns each: its entries carry at most gamma_chunk = 6e-14 of relative error, seven
    orders below the 1e-7 the device is held to (a long-double product of all n^2 m terms takes minutes at m = 8192)."""
    n, m = L.shape
    G = np.eye(n, dtype=LD)
    for c0 in range(0, m, chunk):
        B = L[:, c0:c0 + chunk]
        G += (B @ B.T).astype(LD)
    C = np.zeros((n, n), dtype=LD)
    for j in range(n):                                   # Cholesky, column by column
        C[j, j] = np.sqrt(G[j, j] - C[j, :j] @ C[j, :j])
        if j + 1 < n:
            C[j + 1:, j] = (G[j + 1:, j] - C[j + 1:, :j] @ C[j, :j]) / C[j, j]
    y = np.array(t, dtype=LD)
    for i in range(n):
        y[i] = (y[i] - C[i, :i] @ y[:i]) / C[i, i]
    for i in range(n - 1, -1, -1):
        y[i] = (y[i] - C[i + 1:, i] @ y[i + 1:]) / C[i, i]
    return np.asarray(y @ L.astype(LD), dtype=np.float64)
