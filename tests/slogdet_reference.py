"""The yardstick of the batched slogdet tests: an LU with partial pivoting in np.longdouble (64-bit significand on x86: 2^-11
of a double's rounding unit), vectorised over the batch, and the crafted batches the device kernel is asked to factor.
tests/test_hessian_grid_host.py checks it against numpy on the CPU; tests/test_gpu_slogdet.py and
tests/test_gpu_predict_hessian_multi.py measure the device and LAPACK against it."""
import numpy as np

EPS = 2.0 ** -52
COND_MAX = 1e4          # "well conditioned by construction": random draws above it are redrawn


def slogdet_longdouble(A):
    """(sign float64 (B,), logabsdet longdouble (B,)) of A (B, k, k): row pivot = the first row of maximal |a_ic|, as idamax."""
    a = np.array(A, dtype=np.longdouble)
    B, k, _ = a.shape
    sign, logabs, idx = np.ones(B), np.zeros(B, dtype=np.longdouble), np.arange(B)
    for c in range(k):
        piv = np.argmax(np.abs(a[:, c:, c]), axis=1) + c
        rc, rp = a[idx, c].copy(), a[idx, piv].copy()
        a[idx, c], a[idx, piv] = rp, rc
        sign[piv != c] *= -1.0
        u = a[:, c, c]
        sign = np.where(u == 0, 0.0, sign * np.sign(u).astype(np.float64))
        with np.errstate(divide="ignore"):
            logabs = logabs + np.log(np.abs(u))
        l = a[:, c + 1:, c] / np.where(u == 0, 1, u)[:, None]
        a[:, c + 1:, c + 1:] -= l[:, :, None] * a[:, c, None, c + 1:]
    return sign, logabs


def logdet_errors(A, logabs_device):
    """(max device error, max LAPACK error, the bound 4 max(LAPACK error) + k^2 2^-52) over the nonsingular matrices of the
    batch A (B, k, k), all errors against the longdouble LU."""
    A = np.asarray(A, dtype=np.float64).reshape((-1,) + A.shape[-2:])
    k = A.shape[-1]
    sign, ref = slogdet_longdouble(A)
    ok = sign != 0
    lap = np.linalg.slogdet(A)[1]
    dev = np.asarray(logabs_device, dtype=np.float64).reshape(-1)
    e_dev = float(np.abs(dev[ok] - ref[ok]).max()) if ok.any() else 0.0
    e_lap = float(np.abs(lap[ok] - ref[ok]).max()) if ok.any() else 0.0
    return e_dev, e_lap, 4.0 * e_lap + k * k * EPS


def _well_conditioned(draw, count, seed):
    """`count` matrices from draw(rng, n), those with cond > COND_MAX redrawn from the same seeded stream."""
    rng = np.random.default_rng(seed)
    A = draw(rng, count)
    for _ in range(100):
        bad = np.linalg.cond(A) > COND_MAX
        if not bad.any():
            return A
        A[bad] = draw(rng, int(bad.sum()))
    raise AssertionError("no well-conditioned draw")


def crafted(k, count=200, seed=0):
    """name -> (batch (B, k, k), singular?) for one k.  k = 1 has no odd permutation and no nonsingular matrix with a zero
    leading entry: those two batches start at k = 2; every other batch exists for every k."""
    def gauss(rng, n):
        return rng.normal(size=(n, k, k))

    def sym(rng, n):
        g = rng.normal(size=(n, k, k))
        return g + np.swapaxes(g, 1, 2)

    def zero_lead(rng, n):
        a = rng.normal(size=(n, k, k))
        a[:, 0, 0] = 0.0
        return a

    out = {"gaussian": (_well_conditioned(gauss, count, seed + k), False),
           "symmetric indefinite": (_well_conditioned(sym, count, seed + 100 + k), False),
           "zero matrix": (np.zeros((3, k, k)), True)}
    if k >= 2:
        out["zero leading pivot"] = (_well_conditioned(zero_lead, count, seed + 200 + k), False)
        rng = np.random.default_rng(seed + 300 + k)
        perms = []
        while len(perms) < 20:
            P = np.eye(k)[rng.permutation(k)]
            if round(np.linalg.det(P)) == -1:
                perms.append(P)
        out["odd permutation"] = (np.stack(perms), False)
        rep = rng.normal(size=(count, k, k))
        rep[:, k - 1] = rep[:, 0]
        out["repeated row"] = (rep, True)
    return out
