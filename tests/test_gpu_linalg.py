"""The blocked Cholesky (linalg.hip cholesky_lower_batched, potrf.hip k_potrf128) and the triangular solves on explicitly
inverted 128-blocks (triinv_build, triinv_solve_left, triinv_solve_left_T, triinv_solve_right_T) against a longdouble
yardstick (tests/linalg_reference.py), on every route and block edge, on a real MI355X (-m gpu).

The bounds are fixed by the yardstick, not tuned to the device (tests/test_linalg_reference_host.py shows a float64
emulation of the same design 7 to 3000 times under them):
    Cholesky          max|L L^T - A| / max|A|   <=  4 e_lap + EPS S_blk      (lr.chol_bound)
    triangular solve  max|X - Xref| / max|Xref| <=  4 f_lap + m EPS          (lr.solve_bound)
with e_lap / f_lap LAPACK's own error against the same longdouble reference.  Every case prints the device's error, LAPACK's
and the bound (pytest -s).

Which test pins which branch of the drivers (change the condition and the named test fails or changes route):
    p >= 256 of triinv_solve_left / _left_T        test_trsm at p = 255 | 256 on either side, m >= 129 for the updates
    n < 32768 && m > TB of triinv_solve_right_T    test_right_solve_both_routes: (32767, 257) | (32768, 257), and (200, 128) | (200, 129)
    m > TB of triinv_build                         test_trsm at m = 128 | 129 (without the GEMM pair the blocks below stay zero)
    rem1 <= 0, rem2 <= 0, nb2 < 128, nb1 < 128     test_cholesky_values at m = 128 | 129, 256 | 257, 129 and 385, 257
"""
import re

import numpy as np
import pytest
import scipy.linalg as sla

import linalg_reference as lr
from oracle import mellon_oracle as mo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from mellon_amd import _lib
    return _lib.default_context()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.uint64) == b.view(np.uint64)).all())


def nan_above(M):
    """M with its strict upper triangle replaced by NaN."""
    out = np.array(M, dtype=np.float64)
    out[np.triu_indices_from(out, 1)] = np.nan
    return out


def report(what, dev, lap, bound):
    print(f"\n    {what}: device {dev:.3e}  LAPACK {lap:.3e}  bound {bound:.3e}  ({dev / bound:.3f} of the bound)", end="")


# ---- Cholesky ---------------------------------------------------------------------------------------------------------
_CHOL = [("kernel_like", m) for m in lr.CHOL_SIZES] + [("benign", m) for m in lr.CHOL_BENIGN_SIZES]


@pytest.mark.parametrize("add_diag", [0.0, 1e-6])
@pytest.mark.parametrize("family,m", _CHOL)
def test_cholesky_values(ctx, family, m, add_diag):
    """m = 16, 17: one and two 16-tiles of k_potrf128; 127, 128: one block (rem1 <= 0); 129: nb2 = 1; 255, 256: two blocks
    (rem2 <= 0); 257: a trailing update with rem2 = 1, then a round with nb1 = 1; 384: that round's block is full; 385: a later
    round with nb2 = 1; 513: two full rounds and a third."""
    A, e_lap, s_blk = lr.chol_case(family, m, add_diag)
    L = ctx.chol_lower(A, add_diag=add_diag)
    e_dev = lr.chol_backward(L, A + add_diag * np.eye(m))
    bound = lr.chol_bound(e_lap, s_blk)
    report(f"chol {family} m={m} add_diag={add_diag:g} S_blk={s_blk:.3g}", e_dev, e_lap, bound)
    assert e_dev <= bound
    assert not np.triu(L, 1).any()                                       # the strict upper triangle is exactly zero
    assert same_bits(ctx.chol_lower(A, add_diag=add_diag), L)            # a second call: the same bits


@pytest.mark.parametrize("m", [129, 385])
def test_cholesky_graded_scaling(ctx, m):
    """D A D with D = diag(2^k) is an exact scaling and chol(D A D) = D chol(A): unscaled exactly, the factor of the graded
    matrix (entries over 80 binary orders of magnitude) meets the bound of the ungraded one."""
    A, e_lap, s_blk = lr.chol_case("kernel_like", m, 0.0)
    G, d = lr.graded(A, lr.seed_of("kernel_like", m))
    Lg = ctx.chol_lower(G) / d[:, None]
    e_dev = lr.chol_backward(Lg, A)
    bound = lr.chol_bound(e_lap, s_blk)
    report(f"chol graded m={m}", e_dev, e_lap, bound)
    # (printed, not asserted: every pivot is scaled by a power of four, so bit equality holds if the hardware's
    #  reciprocal-square-root seed is invariant under such a scaling -- which nobody has measured)
    print(f"\n    unscaled factor bit-identical to the factor of A: {same_bits(Lg, ctx.chol_lower(A))}", end="")
    assert e_dev <= bound


@pytest.mark.parametrize("m", [17, 129, 257])
def test_cholesky_reads_the_lower_triangle_only(ctx, m):
    A, _, _ = lr.chol_case("kernel_like", m, 0.0)
    assert same_bits(ctx.chol_lower(nan_above(A)), ctx.chol_lower(A))


@pytest.mark.parametrize("kind", lr.BAD_PIVOT_KINDS)
def test_cholesky_failure_position(ctx, kind):
    """The first bad pivot in the first 16-tile (0, 15), a later tile of the first block (16, 127), the second block column
    (128, 129, 255), a later round (256, 300) and its lone last column (384): the error names pivot k (LAPACK's info - 1,
    tests/test_linalg_reference_host.py), although the host launches the rest of the chain after a failure; and nothing of
    a failed chain is left behind: a good matrix factors to the bound right after the sweep."""
    m = lr.BAD_PIVOT_M
    A, e_lap, s_blk = lr.chol_case("kernel_like", m, 0.0)
    named = {}
    for k in lr.BAD_PIVOT_KS:
        with pytest.raises(ValueError, match="not positively definite"):
            ctx.chol_lower(lr.bad_pivot(A, k, kind))
        msg = ctx.lib.mln_last_error(ctx.handle).decode()
        hit = re.search(r"pivot at index (\d+)$", msg)
        named[k] = int(hit.group(1)) if hit else msg
    print(f"\n    {kind}: pivot -> index named {named}", end="")
    assert named == {k: k for k in lr.BAD_PIVOT_KS}
    e_dev = lr.chol_backward(ctx.chol_lower(A), A)
    report(f"chol m={m} after the {kind} sweep", e_dev, e_lap, lr.chol_bound(e_lap, s_blk))
    assert e_dev <= lr.chol_bound(e_lap, s_blk)


def test_cholesky_deferred_batched_chain(ctx):
    """dev_cholesky_lower2: an implicit fit defers Lp = chol(cov(xu, xu) + jitter I) and the preconditioner's build factors
    it as the SECOND matrix of one batched chain (grid z of the GEMMs, workgroup 1 of k_potrf128, its own Dinv slab and
    info word).  m = 257: two block columns and a round with nb1 = 1.  The oracle's kernel matrix differs from the
    device's by ~1e-13 relative (test_kernel_matrix_leaves grants kernel values 1e-12): that much is added to the bound."""
    from mellon_amd import cov
    n, d, m = 2000, 6, 257
    x = mo.gaussian_mixture(n, d, seed=n + m)
    nn = mo.exact_nn_distances(x)
    xu = x[np.sort(np.random.default_rng(n + m).choice(n, m, replace=False))]
    c = cov.Matern52(mo.compute_ls(nn))
    fit = ctx.fit_prepare(c.lower(d), x, xu, 1e-6, implicit=True)
    V, Vdr = mo.nn_likelihood_constants(nn, d)
    fit.set_likelihood(V, Vdr, mo.compute_mu(nn, d))
    fit.precond_build(1, 0, force=True)
    A = mo.Covariance.from_dict(c.to_dict())(xu, xu) + 1e-6 * np.eye(m)
    Lref = sla.cholesky(A, lower=True)
    e_lap, s_blk = lr.chol_backward(Lref, A), lr.skeel_blocks(Lref)
    Lp = fit.Lp()
    e_dev = lr.chol_backward(Lp, A)
    bound = lr.chol_bound(e_lap, s_blk) + 1e-12
    report(f"chol deferred, batched m={m} S_blk={s_blk:.3g}", e_dev, e_lap, bound)
    assert e_dev <= bound
    assert not np.triu(Lp, 1).any()


# ---- Lf^-1 B and Lf^-T B ------------------------------------------------------------------------------------------------
_TRSM = [("kernel_like", m) for m in lr.TRSM_SIZES] + [("benign_factor", m) for m in lr.TRSM_BENIGN_SIZES]


@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("p", lr.TRSM_RHS)
@pytest.mark.parametrize("family,m", _TRSM)
def test_trsm(ctx, family, m, p, trans):
    """p < 256: left-looking, one product per block row, in place.  p >= 256: right-looking updates against W2 (trans: W),
    then one block-diagonal launch, in place.  m = 63 .. 65, 193: k_trtri64's partial block and k_trtri_merge128 with
    nb2 = 1; m = 128 | 129: triinv_build's GEMM pair; m = 257, 385: a last block of one row."""
    Lf, B, Xref = lr.trsm_case(family, m, trans)
    B, Xref = np.ascontiguousarray(B[:, :p]), Xref[:, :p]
    X = ctx.trsm_lower(Lf, B, trans=trans)
    f_dev = lr.forward_error(X, Xref)
    f_lap = lr.forward_error(lr.lapack_solve(Lf, B, trans), Xref)
    bound = lr.solve_bound(f_lap, m)
    report(f"trsm {family} m={m} p={p} trans={int(trans)}", f_dev, f_lap, bound)
    assert f_dev <= bound
    assert same_bits(ctx.trsm_lower(Lf, B, trans=trans), X)              # in place, and still the same bits twice


@pytest.mark.parametrize("m", [65, 129, 257])
def test_trsm_reads_the_lower_triangle_only(ctx, m):
    for trans in (False, True):
        Lf, B, _ = lr.trsm_case("kernel_like", m, trans)
        for p in lr.TRSM_RHS:
            Bp = np.ascontiguousarray(B[:, :p])
            assert same_bits(ctx.trsm_lower(nan_above(Lf), Bp, trans=trans), ctx.trsm_lower(Lf, Bp, trans=trans)), (p, trans)


# ---- X Lf^-T ------------------------------------------------------------------------------------------------------------
class _PreparedRows:
    """A covariance evaluated block-wise by the binding (Fit.from_blocks) whose values are the rows of a prepared matrix:
    the 'cells' are row numbers."""
    rows_per_block = 8192

    def __init__(self, K):
        self.K = K

    def block(self, rows, xu):
        return self.K[np.asarray(rows)[:, 0].astype(np.int64)]


_right_cache = {}


def _right_case(m):
    """(Lf, K) per m, computed once: the factor of kernel_like(m) and 32768 standard normal rows; a case of n rows uses K[:n]."""
    if m not in _right_cache:
        Lf = sla.cholesky(lr.kernel_like(m, lr.seed_of("kernel_like", m)), lower=True)
        K = np.random.default_rng(m).normal(size=(32768 if m == 257 else 200, m))
        Lf.setflags(write=False)
        K.setflags(write=False)
        _right_cache[m] = (Lf, K)
    return _right_cache[m]


@pytest.mark.parametrize("n,m", [(200, 128), (200, 129), (200, 257), (32768, 257), (32767, 257)])
def test_right_solve_both_routes(ctx, n, m):
    """L = K Lf^-T of an explicit fit (mln_fit_prepare_from_K / _set_K_rows / _finish_K with Lp given).  (200, 128): a single
    block; (200, 129), (200, 257), (32767, 257): right-looking; (32768, 257): the left-looking loop over block columns with
    K = j0 + nb, the smallest n on that side of the threshold.  Rows are independent: a fixed sample of them against the
    longdouble solution, ALL of them against LAPACK at twice the bound (device and LAPACK each within it)."""
    from mellon_amd import _lib
    Lf, K = _right_case(m)
    K = K[:n]
    fit = _lib.Fit.from_blocks(ctx, _PreparedRows(K), np.arange(n)[:, None], np.zeros((m, 1)), 1e-6, Lp=Lf)
    L = fit.L()
    fit.close()
    sample = sorted(set(range(0, n, 509)) | {0, 127, 128, n - 129, n - 128, n - 1})
    assert len(sample) <= 96 and 0 <= sample[0] and sample[-1] == n - 1
    Yref = lr.solve_lower_longdouble(Lf, K[sample].T, False).T
    L_lap = lr.lapack_solve(Lf, K.T, False).T
    f_dev, f_lap = lr.forward_error(L[sample], Yref), lr.forward_error(L_lap[sample], Yref)
    bound = lr.solve_bound(f_lap, m)
    report(f"X Lf^-T n={n} m={m}, {len(sample)} rows", f_dev, f_lap, bound)
    assert f_dev <= bound
    all_rows = float(np.abs(L - L_lap).max() / np.abs(L_lap).max())
    report(f"X Lf^-T n={n} m={m}, all rows against LAPACK", all_rows, f_lap, 2.0 * bound)
    assert all_rows <= 2.0 * bound
