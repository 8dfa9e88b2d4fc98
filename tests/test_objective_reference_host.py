"""CPU checks of tests/objective_reference.py, the yardstick of tests/test_gpu_objective.py: the reference equals exact
rational arithmetic on tiny dyadic problems (both of its summation routes), a float64 evaluation stays inside the bounds
on every GPU case, every mutation that a wrong guard or a swapped operand amounts to moves a checked quantity by more
than a hundred bounds (the proof that the GPU assertions can fail), and the case lists reach every row of the dispatch
table, both edges of every arm and every segment shape."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

import objective_reference as R

LD = np.longdouble


def test_the_long_double_route_is_the_one_in_use_or_the_exact_one_is():
    """Never double against double: a 64-bit significand, or the fsum route (checked below on every machine)."""
    print(f"np.longdouble nmant = {np.finfo(LD).nmant}, exact-sum fallback in use: {not R.EXTENDED}")
    assert R.EXTENDED == (np.finfo(LD).nmant >= 63)
    assert R.reference.__defaults__[-1] == (not R.EXTENDED) and R.reference_f.__defaults__[-2] == (not R.EXTENDED)


# ---- the reference against exact rationals ------------------------------------------------------------------------------
def _taylor_exp(t):
    """exp of a Fraction with |t| <= 24, as a Fraction: exp(t / 16)^16 from 40 exactly summed terms (1e-40 relative)."""
    r = t / 16
    return sum((r ** i) / math.factorial(i) for i in range(41)) ** 16


def _mp_exp(t):
    """The same through mpmath at 200 bits where it is installed."""
    try:
        import mpmath
    except ImportError:
        return _taylor_exp(t)
    with mpmath.workprec(200):
        v = mpmath.exp(mpmath.mpf(t.numerator) / mpmath.mpf(t.denominator))
        return Fraction(int(v.man)) * Fraction(2) ** int(v.exp)


def test_the_two_exact_exponentials_agree():
    for t in (Fraction(-37, 8), Fraction(0), Fraction(5, 4), Fraction(81, 8)):
        assert abs(_taylor_exp(t) / _mp_exp(t) - 1) < Fraction(1, 10 ** 35)


def _to_fraction(x):
    """A long double as an exact Fraction (hi + lo doubles)."""
    x = LD(x)
    hi = float(x)
    return Fraction(hi) + Fraction(float(x - LD(hi)))


def _dyadic_problem(n, m, seed):
    rng = np.random.default_rng(seed)
    L = rng.integers(-12, 13, size=(n, m)) / 8.0
    z = rng.integers(-9, 10, size=m) / 4.0
    V = rng.integers(-8, 9, size=n) / 4.0
    Vdr = rng.integers(-8, 9, size=n) / 4.0
    w = rng.integers(1, 40, size=n) / 2.0
    return L, V, Vdr, -1.25, z, w


def _exact(L, V, Vdr, mu, z, w):
    exp = _mp_exp
    n, m = L.shape
    Lf = [[Fraction(float(v)) for v in row] for row in L]
    zf = [Fraction(float(v)) for v in z]
    f = [sum(Lf[i][j] * zf[j] for j in range(m)) + Fraction(mu) for i in range(n)]
    e = [exp(f[i] + Fraction(float(V[i]))) for i in range(n)]
    a = [Fraction(float(w[i])) * e[i] for i in range(n)]
    lik = sum(a[i] - (f[i] + Fraction(float(Vdr[i]))) for i in range(n))
    g = [sum(Lf[i][j] * (a[i] - 1) for i in range(n)) for j in range(m)]
    h = [sum(Lf[i][j] ** 2 * e[i] for i in range(n)) for j in range(m)]
    return f, lik, g, h


@pytest.mark.parametrize("exact", [False, True], ids=["longdouble", "fsum"])
@pytest.mark.parametrize("n,m", [(1, 1), (2, 3), (5, 2), (6, 6), (3, 5)])
def test_reference_equals_exact_rational_arithmetic(n, m, exact):
    """To long-double rounding (2^-60 of the terms' magnitudes: a few ulps of the 64-bit significand) on the long-double
    route; to a double's (2^-51) on the fsum route -- and inside the route's own bound either way."""
    exact = exact or not R.EXTENDED          # (np.longdouble only a double: the fsum route is the reference, twice)
    L, V, Vdr, mu, z, w = _dyadic_problem(n, m, 7 * n + m)
    f, lik, g, h = _exact(L, V, Vdr, mu, z, w)
    ref = R.reference(L, V, Vdr, mu, z, rows=np.arange(n), w=w, prior=False, exact=exact)
    rel = 2.0 ** (-51 if exact else -60)
    a = [float(x) for x in ref.a]
    scale_f = [float(np.abs(L[i]) @ np.abs(z)) + abs(mu) for i in range(n)]
    for i in range(n):
        assert abs(_to_fraction(ref.f[i]) - f[i]) <= rel * scale_f[i]
        assert abs(_to_fraction(ref.f[i]) - f[i]) <= ref.df[i]
    mag = sum(a[i] + abs(float(f[i])) + abs(Vdr[i]) for i in range(n))
    assert abs(_to_fraction(ref.lik) - lik) <= rel * mag and abs(_to_fraction(ref.lik) - lik) <= ref.dlik
    for j in range(m):
        sg = sum(abs(L[i, j]) * (a[i] + 1.0) for i in range(n))
        sh = sum(L[i, j] ** 2 * float(ref.e[i]) for i in range(n))
        assert abs(_to_fraction(ref.grad[j]) - g[j]) <= rel * sg and abs(_to_fraction(ref.grad[j]) - g[j]) <= ref.dgrad[j]
        assert abs(_to_fraction(ref.hess[j]) - h[j]) <= rel * sh and abs(_to_fraction(ref.hess[j]) - h[j]) <= ref.dhess[j]
    # the prior terms
    full = R.reference(L, V, Vdr, mu, z, exact=exact)
    plain = R.reference(L, V, Vdr, mu, z, prior=False, exact=exact)
    zz = sum(Fraction(float(v)) ** 2 for v in z) / 2
    assert abs(_to_fraction(full.loss - plain.lik) - zz - Fraction(m * math.log(2 * math.pi) / 2)) < 1e-14 * (1 + m)
    assert np.array_equal(np.asarray(full.grad - plain.grad, dtype=np.float64), z)
    assert np.array_equal(np.asarray(full.hess - plain.hess, dtype=np.float64), np.ones(m))


def test_two_prod_is_error_free():
    rng = np.random.default_rng(3)
    a, b = rng.normal(size=200), rng.normal(size=200)
    p, e = R._two_prod(a, b)
    for i in range(200):
        assert Fraction(p[i]) + Fraction(e[i]) == Fraction(a[i]) * Fraction(b[i])


# ---- bounds: valid for a float64 evaluation, and far below every mutation ----------------------------------------------
CASES = sorted(set(R.VALUE_CASES))


@functools.lru_cache(maxsize=None)
def _case(n, m):
    """Everything the two tests below need of one case, computed once: ratios of the float64 evaluation, and of each
    mutated float64 evaluation, to the bounds."""
    L, V, Vdr, mu, z = R.make_problem(n, m, R.case_seed(n, m))
    ref = R.reference(L, V, Vdr, mu, z)

    def ratios(loss, grad, hess, f, rows=slice(None)):
        return {"loss": R.ratio(loss, ref.loss, ref.dloss), "grad": R.ratio(grad, ref.grad, ref.dgrad),
                "hess": R.ratio(hess, ref.hess, ref.dhess), "f": R.ratio(f, ref.f[rows], ref.df[rows])}

    out = {"plain": ratios(*R.evaluate64(L, V, Vdr, mu, z))}
    if n * m <= 1 << 21:        # z = 0 (the loss is then the constant (m / 2) log 2 pi plus a few row terms)
        z0 = np.zeros(m)
        ref0 = R.reference(L, V, Vdr, mu, z0, hess=False)
        l0, g0, _, f0 = R.evaluate64(L, V, Vdr, mu, z0)
        out["plain z=0"] = {"loss": R.ratio(l0, ref0.loss, ref0.dloss), "grad": R.ratio(g0, ref0.grad, ref0.dgrad),
                            "f": R.ratio(f0, ref0.f, ref0.df)}
    if n < 2 or m < 2:
        return out
    # the last row dropped (its f is not compared: it does not exist)
    l1, g1, h1, f1 = R.evaluate64(L[:-1], V[:-1], Vdr[:-1], mu, z)
    out["last row dropped"] = ratios(l1, g1, h1, f1, slice(0, n - 1))
    # the last column never read: its z counts as 0 in f, its gradient and Hessian partials stay 0
    Lc = L.copy()
    Lc[:, -1] = 0.0
    out["last column dropped"] = ratios(*R.evaluate64(Lc, V, Vdr, mu, z))
    # z[m - 1] read as zero by the kernel (the prior terms are the host's and keep the real z)
    zc = z.copy()
    zc[-1] = 0.0
    l3, g3, h3, f3 = R.evaluate64(L, V, Vdr, mu, zc)
    out["z[m-1] zeroed"] = ratios(l3 + 0.5 * z[-1] ** 2, g3 + (z - zc), h3, f3)
    out["V and Vdr swapped"] = ratios(*R.evaluate64(L, Vdr, V, mu, z))
    nseg = len(R.segments(m))
    if nseg > 1:                                        # (one launch adds mu once by construction)
        l5, g5, h5, f5 = R.evaluate64(L, V, Vdr, nseg * mu, z)
        out["mu added once per segment"] = ratios(l5, g5, h5, f5)
    out["L rounded to fp32"] = ratios(*R.evaluate64(L.astype(np.float32).astype(np.float64), V, Vdr, mu, z))
    # the weight on the -f term as well: against the weighted reference (row-wise, from the f already computed)
    w = np.exp(np.random.default_rng(n + m).uniform(0.0, math.log(1e4), size=n))
    lik, dlik, *_ = R.lik_and_bound(ref.f, ref.df, V, Vdr, w)
    f64 = np.asarray(ref.f, dtype=np.float64)
    e64 = np.exp(f64 + V)
    out["weighted plain"] = {"lik": R.ratio((w * e64 - (f64 + Vdr)).sum(), lik, dlik)}
    out["weight on the -f term too"] = {"lik": R.ratio((w * (e64 - (f64 + Vdr))).sum(), lik, dlik)}
    return out


@pytest.mark.parametrize("n,m", CASES)
def test_a_float64_evaluation_is_inside_one_bound(n, m):
    r = _case(n, m)
    print(n, m, {k: f"{v:.3f}" for k, v in r["plain"].items()})
    assert max(r["plain"].values()) < 1.0, r["plain"]
    if "plain z=0" in r:
        assert max(r["plain z=0"].values()) < 1.0, r["plain z=0"]
    if "weighted plain" in r:
        assert r["weighted plain"]["lik"] < 1.0


@pytest.mark.parametrize("n,m", [c for c in CASES if c[0] >= 2 and c[1] >= 2])
def test_every_mutation_moves_a_checked_quantity_by_a_hundred_bounds(n, m):
    """The mutated evaluations are float64 (inside one bound of their own exact value, see above): more than 101 bounds
    from the reference is more than 100 for the mutation itself."""
    r = _case(n, m)
    wanted = {"last row dropped", "last column dropped", "z[m-1] zeroed", "V and Vdr swapped", "L rounded to fp32",
              "weight on the -f term too"} | ({"mu added once per segment"} if m > R.SEG else set())
    assert wanted <= set(r)
    for name in wanted:
        assert max(r[name].values()) > 101.0, (name, r[name])


# ---- coverage of the dispatch -------------------------------------------------------------------------------------------
def test_dispatch_restatement():
    assert R.variant(1, "obj") == (1, 8, True) and R.variant(1024, "gemvt") == (1, 8, False)
    assert R.variant(1025, "hess") == (2, 8, True) and R.variant(2048, "fonly") == (2, 5, False)
    assert R.variant(2049, "obj") == (3, 4, True) and R.variant(3072, "gemvt") == (3, 3, False)
    for m, c in ((3073, 4), (4096, 4), (4097, 5), (5120, 5), (5121, 6), (6144, 6)):
        for mode in R.MODES:
            assert R.variant(m, mode) == (c, 2, False)
    for m in (6145, 7168, 7169, 8192):
        for mode in R.MODES:
            assert R.variant(m, mode) == (8, 1, False)
    # pad16: m = 1009 .. 1024 share a leading dimension, 1025 is the next arm
    assert R.cpt_of(1009) == R.cpt_of(1024) == 1 and R.cpt_of(1025) == 2
    # a segment is sized by its own columns, not by the padded pitch
    assert R.cpt_of(1025, segment=True) == 2 and R.cpt_of(1024, segment=True) == 1 and R.cpt_of(1, segment=True) == 1
    assert R.segments(8192) == []
    assert R.segments(8193) == [(0, 8192, 4104, 8192), (8192, 1, 8, 2)]
    assert R.segments(8194) == [(0, 8192, 4104, 8192), (8192, 2, 8, 2)]
    assert [s[1] for s in R.segments(9217)] == [8192, 1025] and R.segments(9217)[1][3] == 1026
    assert [s[1] for s in R.segments(16384)] == [8192, 8192]
    assert [s[1] for s in R.segments(16385)] == [8192, 8192, 1]
    assert R.launches(9217, "objective") == [(8, 1, False), (2, 5, False)] * 2
    assert R.launches(8193, "objective_hess") is None and R.launches(8193, "rows") is None


def test_case_lists_reach_every_row_of_the_dispatch_table():
    fused = {v for v in R._FUSED.values()}
    plain = {v for v in R._PLAIN.values()}
    ms = sorted({m for _, m in R.VALUE_CASES})
    assert ms == sorted(R.M_EDGES)
    one_pass = [m for m in ms if m <= R.SEG]
    assert {R.variant(m, "obj") for m in one_pass} == fused               # objective(z)
    assert {R.variant(m, "hess") for m in one_pass} == fused              # objective(z, with_hess=True)
    assert {R.variant(m, "fonly") for m in one_pass} == plain             # transform
    assert {R.cpt_of(m) for m in one_pass} == set(range(1, 9))            # 7 and 8 both, though they share <8, 1>
    assert {R.variant(m, "gemvt") for m in R.RIDGE_M if m <= R.SEG} | {(1, 8, False)} == plain   # ridge_init, cpt >= 2
    assert {R.variant(m, "obj") for m in R.ROWS_M} == fused               # KEEP / strided / LIST
    assert {R.cpt_of(m) for m in R.ROWS_M} == {1, 2, 3, 4, 5, 6, 7, 8}
    # both edges of every pad16(m) interval
    for c in range(1, 9):
        lo, hi = 1024 * (c - 1) + 1, 1024 * c
        assert hi in ms and (lo in ms), (lo, hi)
        assert R.cpt_of(lo) == c == R.cpt_of(hi)
    assert 8191 in ms and {1, 2, 3, 16, 17} <= set(ms)                    # odd m, one pair, the first pad16 edge
    # segment shapes: a last segment of one column, an odd and an even last segment, one that needs CPT = 2, three segments
    last = {m: R.segments(m)[-1] for m in ms if m > R.SEG}
    assert last[8193][1] == 1 and last[8193][2] == 8
    assert last[8194][1] == 2 and last[16384][1] == 8192
    assert R.cpt_of(last[9217][1], True) == 2 and last[9217][1] % 2 == 1
    assert len(R.segments(16385)) == 3 and last[16385][1] == 1
    # n = 2057 at the first m of every cpt and at 8193; every other n everywhere
    for m in ms:
        ns = sorted(n for n, mm in R.VALUE_CASES if mm == m)
        assert ns == sorted(set(R.N_EDGES + [R.N_EXACT]) - (set() if m in R.M_LOWER else {2057})), m
    assert [R.cpt_of(m) for m in R.M_LOWER[:-1]] == list(range(1, 9)) and R.M_LOWER[-1] == 8193
    assert all(R.cpt_of(m - 1) == R.cpt_of(m) - 1 for m in R.M_LOWER[1:-1])
    assert max(n * m for n, m in R.VALUE_CASES) == 2057 * 8193 and max(m for _, m in R.VALUE_CASES) == 16385


def test_row_counts_reach_every_row_edge():
    ns = R.N_EDGES + [R.N_EXACT]
    assert 1 in ns
    for Rr in (8, 5, 4, 3, 2, 1):
        if Rr > 1:
            assert any(n < Rr for n in ns)                                       # fewer rows than a step
        assert any(n > Rr and n % Rr for n in ns) or Rr == 1                     # ragged last step
        assert any(n >= Rr and n % Rr == 0 for n in ns)                          # exact last step
        assert any(R.row_split(n, Rr)[0] < 16 for n in ns)                       # empty groups in k_reduce_obj
        big = [R.row_split(n, Rr) for n in (533, 2057)]
        assert all(nw == R.N_CU for nw, _ in big)
        counts = {s for _, steps in big for s in steps if s}
        assert any(s % 2 for s in counts) and any(s % 2 == 0 for s in counts)    # the `if (s + 1 < s_end)` tail, and not
        assert max(steps.count(0) for _, steps in big) >= 27                     # workgroups with no rows at all
    assert all(max(R.row_split(n, Rr)[1].count(0) for n in (533, 2057)) > 100 for Rr in (8, 5, 4, 2))
    # the row maps: counts below, at and above a step of every R, fewer rows than workgroups, ragged last workgroup
    assert {1, 7, 8, 9, 17, 255, 257, 700, 1000} == set(R.ROWS_COUNTS)
    for count in R.ROWS_COUNTS:
        ps = R.progressions(count)
        assert any(first + (count - 1) * stride == R.ROWS_N - 1 for first, stride in ps)
        assert all(0 <= first and first + (count - 1) * stride < R.ROWS_N for first, stride in ps)
    assert any(stride > 1 for count in R.ROWS_COUNTS for _, stride in R.progressions(count))
