"""CPU checks of tests/linalg_reference.py, the yardstick of tests/test_gpu_linalg.py: the longdouble substitution against
scipy, the residual against LAPACK's own factor, the crafted failures against LAPACK's failure index -- and that the two
bounds the device is held to are REACHABLE by its design: a plain-NumPy emulation of the blocked factorisation and of both
routes of every solve, in float64 building blocks, meets them on every crafted case (margins printed, pytest -s)."""
import numpy as np
import pytest
import scipy.linalg as sla

import linalg_reference as lr


def test_longdouble_is_wider_than_double():
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


@pytest.mark.parametrize("trans", [False, True])
def test_longdouble_solve_agrees_with_scipy(trans):
    Lf = lr.benign_factor(40, 1)
    B = np.random.default_rng(2).normal(size=(40, 5))
    X = lr.solve_lower_longdouble(Lf, B, trans)
    assert X.dtype == np.longdouble
    assert lr.forward_error(lr.lapack_solve(Lf, B, trans), X) < 1e-12
    # only the lower triangle is read; a vector stays a vector
    poisoned = Lf + np.triu(np.full((40, 40), np.nan), 1)
    assert np.array_equal(lr.solve_lower_longdouble(poisoned, B, trans), X)
    assert np.array_equal(lr.solve_lower_longdouble(Lf, B[:, 0], trans), X[:, 0])


def test_chol_backward_of_lapack_factor():
    A = lr.benign(100, 3)
    L = sla.cholesky(A, lower=True)
    assert lr.chol_backward(L, A) < 64 * lr.EPS
    # lower triangle only, of both arguments
    nan_up = np.triu(np.full((100, 100), np.nan), 1)
    assert lr.chol_backward(L + nan_up, A + nan_up) == lr.chol_backward(L, A)
    # and it does see an error: one entry off by 1e-10
    L2 = L.copy()
    L2[70, 30] += 1e-10
    assert lr.chol_backward(L2, A) > 1e-12


def test_skeel_blocks_and_forward_error():
    assert lr.skeel_blocks(np.eye(300) * 3.0) == 1.0
    T = np.array([[1.0, 0.0], [-4.0, 1.0]])                 # T^-1 = [[1, 0], [4, 1]]: |T^-1| |T| = [[1, 0], [8, 1]]
    assert lr.skeel_blocks(T) == 9.0
    big = np.eye(130)
    big[129, 128] = -4.0                                    # the second 128-block is 2 x 2
    assert lr.skeel_blocks(big) == 9.0 and lr.skeel_blocks(big, nb=129) == 1.0
    assert lr.forward_error(np.array([1.0, 2.0 + 2.0 ** -40]), np.array([1.0, 2.0])) == 2.0 ** -41


def test_graded_scaling_is_exact():
    A = lr.kernel_like(129, 5)
    G, d = lr.graded(A, 6)
    assert np.array_equal(G / d[:, None] / d[None, :], A)
    assert set(np.log2(d)) <= set(range(-20, 21)) and len(set(d)) > 10


@pytest.mark.parametrize("kind", lr.BAD_PIVOT_KINDS)
def test_crafted_failures_fail_where_the_device_must_report(kind):
    """LAPACK's dpotrf fails at pivot k (info = k + 1) on every crafted failure.  NaN pivots: LAPACK's dpotf2 tests
    `ajj <= 0 or isnan(ajj)`, but a LAPACK whose potrf is the BLAS vendor's own may test `ajj <= 0` alone and sail through
    a NaN with info = 0; there the same fact is shown in its parts: the leading k x k block factors (pivots 0 .. k-1 are
    positive), and the unblocked algorithm with LAPACK's test stops at k.  A failure index other than k + 1 is never
    accepted."""
    A = lr.make_matrix("kernel_like", lr.BAD_PIVOT_M)
    assert sla.lapack.dpotrf(A, lower=1)[1] == 0
    for k in lr.BAD_PIVOT_KS:
        bad = lr.bad_pivot(A, k, kind)
        assert np.array_equal(bad[:k, :k], A[:k, :k])
        assert lr.first_bad_pivot(bad) == k
        info = sla.lapack.dpotrf(bad, lower=1)[1]
        if kind == "negative" or info != 0:
            assert info == k + 1, (kind, k, info)
        else:
            assert k == 0 or sla.lapack.dpotrf(bad[:k, :k], lower=1)[1] == 0
            assert np.isnan(bad[k, k]) and np.isfinite(np.delete(bad.ravel(), k * (lr.BAD_PIVOT_M + 1))).all()


def _chol_cases():
    for m in lr.CHOL_SIZES:
        for add_diag in (0.0, 1e-6):
            yield "kernel_like", m, add_diag
    for m in lr.CHOL_BENIGN_SIZES:
        for add_diag in (0.0, 1e-6):
            yield "benign", m, add_diag


def test_cholesky_bound_is_reachable_by_the_blocked_design():
    """Diagonal blocks factored, inverted by substitution, panel = A21 X^T, trailing update -- all in float64: the
    emulation meets 4 e_lap + EPS S_blk on every case of the GPU test, the graded ones and a harder jitter."""
    worst = 0.0
    print()
    cases = list(_chol_cases()) + [("kernel_like 1e-9", m, 0.0) for m in (129, 257, 385, 513)]
    for family, m, add_diag in cases:
        if family == "kernel_like 1e-9":
            A = lr.kernel_like(m, lr.seed_of("kernel_like", m), jitter=1e-9)
            Lref = sla.cholesky(A, lower=True)
            e_lap, s_blk = lr.chol_backward(Lref, A), lr.skeel_blocks(Lref)
        else:
            A, e_lap, s_blk = lr.chol_case(family, m, add_diag)
        Afull = A + add_diag * np.eye(m)
        e_emu = lr.chol_backward(lr.emulate_cholesky(Afull), Afull)
        bound = lr.chol_bound(e_lap, s_blk)
        print(f"chol {family:>16} m={m:<4} add_diag={add_diag:<6g} emulation {e_emu:.2e}  LAPACK {e_lap:.2e}  "
              f"S_blk {s_blk:.3g}  bound {bound:.2e}  margin x{bound / e_emu:.1f}")
        assert e_emu <= bound
        worst = max(worst, e_emu / bound)
    for m in (129, 385):
        A, e_lap, s_blk = lr.chol_case("kernel_like", m, 0.0)
        G, d = lr.graded(A, lr.seed_of("kernel_like", m))
        e_emu = lr.chol_backward(lr.emulate_cholesky(G) / d[:, None], A)
        bound = lr.chol_bound(e_lap, s_blk)
        print(f"chol graded kernel_like m={m:<4} emulation {e_emu:.2e}  bound {bound:.2e}  margin x{bound / e_emu:.1f}")
        assert e_emu <= bound
    assert worst < 1.0


def test_solve_bound_is_reachable_by_both_routes():
    """Left-looking and right-looking, forward and transposed, every (m, p) of the GPU test: the emulation meets
    4 f_lap + m EPS whichever route the device takes at that p."""
    print()
    cases = [("kernel_like", m) for m in lr.TRSM_SIZES] + [("benign_factor", m) for m in lr.TRSM_BENIGN_SIZES]
    for family, m in cases:
        for trans in (False, True):
            Lf, B, Xref = lr.trsm_case(family, m, trans)
            copies = lr.block_scaled_copies(Lf)
            line = []
            for p in lr.TRSM_RHS:
                f_lap = lr.forward_error(lr.lapack_solve(Lf, B[:, :p], trans), Xref[:, :p])
                bound = lr.solve_bound(f_lap, m)
                for right_looking in (False, True):
                    f_emu = lr.forward_error(lr.emulate_solve(copies, B[:, :p], trans, right_looking), Xref[:, :p])
                    assert f_emu <= bound, (family, m, p, trans, right_looking, f_emu, f_lap, bound)
                    line.append(bound / max(f_emu, 1e-300))
            print(f"trsm {family:>13} m={m:<4} trans={int(trans)}  smallest margin over p and both routes x{min(line):.1f}")


@pytest.mark.parametrize("m", [128, 129, 257])
def test_right_solve_bound_is_reachable_by_both_routes(m):
    """X Lf^-T, rows independent: both routes of the emulation against the longdouble solution of Lf Y = X^T."""
    Lf = sla.cholesky(lr.kernel_like(m, lr.seed_of("kernel_like", m)), lower=True)
    X = np.random.default_rng(m).normal(size=(200, m))
    Yref = lr.solve_lower_longdouble(Lf, X.T, False).T
    f_lap = lr.forward_error(lr.lapack_solve(Lf, X.T, False).T, Yref)
    bound = lr.solve_bound(f_lap, m)
    copies = lr.block_scaled_copies(Lf)
    print()
    for right_looking in (False, True):
        f_emu = lr.forward_error(lr.emulate_solve_right_T(copies, X, right_looking), Yref)
        print(f"X Lf^-T m={m:<4} right_looking={int(right_looking)} emulation {f_emu:.2e}  LAPACK {f_lap:.2e}  bound {bound:.2e}")
        assert f_emu <= bound


def test_emulated_routes_solve_the_same_system():
    """The two routes are rearrangements of one substitution: on a small-block instance (nb = 4, every edge in play) they
    agree with scipy to rounding, so the emulation above emulates a solve and not something else."""
    rng = np.random.default_rng(0)
    Lf = lr.benign_factor(11, 0)
    B = rng.normal(size=(11, 3))
    for trans in (False, True):
        ref = lr.lapack_solve(Lf, B, trans)
        for right_looking in (False, True):
            assert np.abs(lr.emulate_solve(lr.block_scaled_copies(Lf, 4), B, trans, right_looking, nb=4) - ref).max() < 1e-13
    X = rng.normal(size=(5, 11))
    for right_looking in (False, True):
        assert np.abs(lr.emulate_solve_right_T(lr.block_scaled_copies(Lf, 4), X, right_looking, nb=4) - lr.lapack_solve(Lf, X.T, False).T).max() < 1e-13
    A = lr.benign(11, 1)
    assert np.abs(lr.emulate_cholesky(A, nb=4) - sla.cholesky(A, lower=True)).max() < 1e-13
