"""The objective pass (csrc/objective.hip, k_objective<CPT, R, MODE, KEEP, VEC, LIST>) on a real MI355X (-m gpu), on every
specialisation, mode and row map, against the long-double reference and the order-independent forward-error bounds of
tests/objective_reference.py (checked on the CPU by tests/test_objective_reference_host.py: a dropped row or column, a
swapped operand or an fp32 rounding of L moves a checked quantity by more than a hundred bounds).

All handles come from Fit.from_L + set_likelihood: no kernel matrix, no k-means.  A result passes when
|got - ref| <= 2 x bound element by element; every case prints its worst error / bound (pytest -s), and the module prints
the worst per quantity when it is done.

Dispatch (launch_objective; restated and pinned in objective_reference.variant / segments):
    cpt = ceil(pad16(m) / 1024):  1 <1,8,VEC> | <1,8>,  2 <2,8,VEC> | <2,5>,  3 <3,4,VEC> | <3,3>,  4..6 <cpt,2>,  7, 8 <8,1>
    (OBJ and OBJ_HESS | GEMVT and FONLY); beyond 8192 columns: FONLY per 8192-column segment with f_accum, k_lik_rows,
    GEMVT per segment.  n_wg = min(n_cu, (n + 1) / 2), nsteps = ceil(n / R), per = ceil(nsteps / n_wg).
"""
import types

import numpy as np
import pytest

import objective_reference as R

pytestmark = pytest.mark.gpu

LIMIT = 2.0                       # a device result may be 2 x bound from the reference (objective_reference's docstring)
WORST = {}


def _note(quantity, value):
    WORST[quantity] = max(WORST.get(quantity, 0.0), value)
    return value


def _check(tag, pairs):
    """pairs: (quantity, got, ref, bound).  Prints every ratio before asserting any."""
    rs = {q: _note(q, R.ratio(got, ref, bound)) for q, got, ref, bound in pairs}
    print(f"{tag}: " + ", ".join(f"{q} {v:.3f}" for q, v in rs.items()))
    bad = {q: v for q, v in rs.items() if not v <= LIMIT}
    assert not bad, (tag, bad)


@pytest.fixture(scope="module")
def ctx():
    from mellon_amd import _lib
    c = _lib.default_context()
    print("device:", c.device_info())
    yield c
    print("\nworst error / bound per quantity (ridge z0: relmax):", {k: float(f"{v:.3g}") for k, v in sorted(WORST.items())})


def _handle(ctx, n, m):
    from mellon_amd import _lib
    L, V, Vdr, mu, z = R.make_problem(n, m, R.case_seed(n, m))
    fit = _lib.Fit.from_L(ctx, L)
    fit.set_likelihood(V, Vdr, mu)
    return types.SimpleNamespace(fit=fit, L=L, V=V, Vdr=Vdr, mu=mu, z=z, n=n, m=m)


# ---- (a) values, (b) reproducibility: every (n, m) --------------------------------------------------------------------
@pytest.fixture(scope="module", params=R.VALUE_CASES, ids=lambda c: f"n{c[0]}-m{c[1]}")
def problem(request, ctx):
    p = _handle(ctx, *request.param)
    yield p
    p.fit.close()


def test_values(problem):
    """objective(z), objective(z, with_hess=True), transform (with the likelihood's mu and with another) and objective(0)
    inside 2 x bound; beyond 8192 columns the Hessian diagonal is refused, not returned."""
    p = problem
    tag = f"n={p.n} m={p.m}"
    ref = R.reference(p.L, p.V, p.Vdr, p.mu, p.z, hess=p.m <= R.SEG)
    loss, grad = p.fit.objective(p.z)
    pairs = [("loss", loss, ref.loss, ref.dloss), ("grad", grad, ref.grad, ref.dgrad)]
    if p.m <= R.SEG:
        lh, gh, hh = p.fit.objective(p.z, with_hess=True)
        pairs += [("loss (hess pass)", lh, ref.loss, ref.dloss), ("grad (hess pass)", gh, ref.grad, ref.dgrad),
                  ("hess", hh, ref.hess, ref.dhess)]
    else:
        with pytest.raises(NotImplementedError, match="not available beyond 8192"):
            p.fit.objective(p.z, with_hess=True)
    pairs.append(("f", p.fit.transform(p.z, p.mu), ref.f, ref.df))
    f2, df2 = R.reference_f(p.L, p.z, 1.25)
    pairs.append(("f (other mu)", p.fit.transform(p.z, 1.25), f2, df2))
    z0 = np.zeros(p.m)
    ref0 = R.reference(p.L, p.V, p.Vdr, p.mu, z0, hess=False)
    l0, g0 = p.fit.objective(z0)
    pairs += [("loss (z = 0)", l0, ref0.loss, ref0.dloss), ("grad (z = 0)", g0, ref0.grad, ref0.dgrad)]
    _check(tag, pairs)


def test_two_calls_give_the_same_bits(problem):
    p = problem
    a, b = p.fit.objective(p.z), p.fit.objective(p.z)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    assert np.array_equal(p.fit.transform(p.z, p.mu), p.fit.transform(p.z, p.mu))
    if p.m > R.SEG:
        return
    ha, hb = p.fit.objective(p.z, with_hess=True), p.fit.objective(p.z, with_hess=True)
    assert ha[0] == hb[0] and np.array_equal(ha[1], hb[1]) and np.array_equal(ha[2], hb[2])
    same = ha[0] == a[0] and np.array_equal(ha[1], a[1])
    if R.cpt_of(p.m) == 1:            # asserted since test_fit_pipeline_sparse; on the other arms it is only reported
        assert same
    else:
        print(f"n={p.n} m={p.m} cpt={R.cpt_of(p.m)}: objective(z) has the bits of objective(z, with_hess=True): {same}")


# ---- (c) GEMVT through ridge_init ------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", R.RIDGE_M)
def test_ridge_start(ctx, m):
    """z0 = (L^T L + I)^-1 L^T t against L^T (L L^T + I)^-1 t in long double.  1e-7 is the project's figure for this
    quantity (test_fit_pipeline_sparse): the preconditioner's Cholesky sits between the kernel and the result; a dropped
    row moves z0 by about 1e-3."""
    p = _handle(ctx, R.RIDGE_N, m)
    try:
        t = np.random.default_rng(m).normal(size=p.n)
        z0 = p.fit.ridge_init(t)
    finally:
        p.fit.close()
    want = R.ridge_reference(p.L, t)
    err = np.abs(z0 - want).max() / np.abs(want).max()
    _note("ridge z0 relmax", err)
    print(f"m={m} {R.launches(m, 'gemvt')}: relmax {err:.2e}")
    assert err < 1e-7


# ---- (d) row maps ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=R.ROWS_M, ids=lambda m: f"m{m}")
def rows_problem(request, ctx):
    p = _handle(ctx, R.ROWS_N, request.param)
    yield p
    p.fit.close()


def _rows_ref(p, rows, w=None):
    return R.reference(p.L, p.V, p.Vdr, p.mu, p.z, rows=rows, w=w, hess=False, prior=False)


def _rows_pairs(ref, got, scale=0.0, suffix=""):
    lik, dlik, g, dg = ref.lik, ref.dlik, ref.grad, ref.dgrad
    if scale != 0.0:
        (lik, dlik), (g, dg) = R.scaled(lik, dlik, scale), R.scaled(g, dg, scale)
    loss, grad, f = got
    return [("rows lik" + suffix, loss, lik, dlik), ("rows grad" + suffix, grad, g, dg), ("rows f" + suffix, f, ref.f, ref.df)]


@pytest.mark.parametrize("count", R.ROWS_COUNTS)
def test_strided_rows_and_the_list_over_the_same_rows(rows_problem, count):
    """Every progression, with and without out_scale, inside the bounds; the list launch over the same rows returns the
    bits of the strided one (test_a_progression_list_equals_the_strided_launch, on every arm)."""
    p = rows_problem
    for first, stride in R.progressions(count):
        rows = first + stride * np.arange(count, dtype=np.int64)
        pairs, ref = [], _rows_ref(p, rows)
        for scale in (0.0, 3.0):
            got = p.fit.objective_rows(p.z, count=count, first=first, stride=stride, out_scale=scale)
            lst = p.fit.objective_rows(p.z, rows=rows, out_scale=scale)
            assert lst[0] == got[0] and np.array_equal(lst[1], got[1]) and np.array_equal(lst[2], got[2]), (first, stride, scale)
            pairs += _rows_pairs(ref, got, scale=scale, suffix=" (scaled)" if scale else "")
        _check(f"m={p.m} {R.variant(p.m, 'obj')} count={count} first={first} stride={stride}", pairs)


@pytest.mark.parametrize("count", R.ROWS_COUNTS)
def test_a_weighted_random_list(rows_problem, count):
    p = rows_problem
    rng = np.random.default_rng(1000 * p.m + count)
    rows = np.sort(rng.choice(R.ROWS_N, size=count, replace=False)).astype(np.int64)
    w = np.exp(rng.uniform(0.0, np.log(1e4), size=count))
    got = p.fit.objective_rows(p.z, rows=rows, weights=w)
    _check(f"m={p.m} count={count} weighted list", _rows_pairs(_rows_ref(p, rows, w), got, suffix=" (weighted)"))
    one = p.fit.objective_rows(p.z, rows=rows, weights=np.ones(count))
    none = p.fit.objective_rows(p.z, rows=rows)
    assert one[0] == none[0] and np.array_equal(one[1], none[1]) and np.array_equal(one[2], none[2])
    _check(f"m={p.m} count={count} plain list", _rows_pairs(_rows_ref(p, rows), none))


def test_row_maps_are_refused_beyond_8192_columns(ctx):
    p = _handle(ctx, 10, 8193)
    try:
        with pytest.raises(NotImplementedError):
            p.fit.objective_rows(p.z, count=4, first=1, stride=2)
        with pytest.raises(NotImplementedError):
            p.fit.objective_rows(p.z, rows=np.array([0, 3, 9], dtype=np.int64))
    finally:
        p.fit.close()


# ---- (e) overflow is not hidden --------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", R.OVERFLOW_M)
def test_overflow_comes_back_as_it_is(ctx, m):
    """One row with t = f + V = 710 (exp overflows at 709.78): the loss is +inf, the gradient is sign(L_ij) inf in every
    column ("a non-finite loss is returned as it comes", include/mellon_hip.h); f does not depend on V and stays inside
    its bound."""
    from mellon_amd import _lib
    n, row = R.OVERFLOW_N, 3
    L, V, Vdr, mu, z = R.make_problem(n, m, R.case_seed(n, m))
    assert (L[row] != 0.0).all()
    f, df = R.reference_f(L, z, mu)
    V = V.copy()
    V[row] = 710.0 - float(f[row])
    fit = _lib.Fit.from_L(ctx, L)
    try:
        fit.set_likelihood(V, Vdr, mu)
        loss, grad = fit.objective(z)
        got_f = fit.transform(z, mu)
    finally:
        fit.close()
    print(f"m={m}: loss {loss}, gradient entries +inf {np.isposinf(grad).sum()} -inf {np.isneginf(grad).sum()} of {m}")
    assert loss == np.inf
    assert np.array_equal(grad, np.sign(L[row]) * np.inf)
    _check(f"m={m} overflow", [("f", got_f, f, df)])
