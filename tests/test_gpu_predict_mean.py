"""The fused predictive mean (mln_predict_mean, one output column) on every dispatch path of launch_predict_mean1
(csrc/cov_kernels.hip) against the extended-precision restatement (tests/predict_restatement.py), on a real MI355X
(-m gpu):

  A  k_predict_mean_rows<KIND, KSTEPS>  one stationary leaf over all d <= 64 columns, n >= 4096, m >= 256
  B  launch_predict_mean_rows_prod      the time-sensitive product kernel (test_product_kernel_predict_rows)
  C  k_predict_mean_mfma                one leaf over all columns, n m >= 4096, otherwise (any d)
  D  k_predict_mean1<true>              one leaf, anything else
  E  k_predict_mean1<false>             composite programs

Every comparison is per row:
  |got_i - mean_i| <= TOLK sum_{j not in co(i)} |w_j| + TOLCO sum_{j in co(i)} |w_j| + (m + 64) 2^-53 sum_j |K_ij w_j|
with co(i) the centres closer than 0.05 to cell i (predict_restatement.row_bound; the tolerances and their measurement
against the oracle: test_predict_restatement_host.py)."""
import functools

import numpy as np
import pytest

import predict_restatement as pr
from test_predict_restatement_host import TOLCO, TOLK

pytestmark = pytest.mark.gpu

LD = np.longdouble
ROW_KINDS = ("Matern32", "Matern52", "ExpQuad", "Exponential", "RatQuad")
MU = 0.25


@pytest.fixture(scope="module")
def mellon():
    import mellon_amd
    return mellon_amd


@pytest.fixture(scope="module")
def ctx():
    from mellon_amd import _lib
    return _lib.default_context()


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=2)
def _problem(kind, d, n, m, seed, m_extra=0):
    """Inputs of the recipe and their longdouble kernel matrix, computed once per parameter set and shared read-only.
    m_extra: further plain centres behind the recipe's m, so that every prefix of at least m centres holds all of the
    recipe's coincident and near centres."""
    x, y, w = pr.make_inputs(n, m, d, seed)
    if m_extra:
        rng = np.random.default_rng(seed + 1)
        y = np.concatenate([y, rng.normal(size=(m_extra, d)) * 1.5])
        w = np.concatenate([w, rng.normal(size=m_extra)])
    params = pr.kind_params(kind, d)
    K, dist = pr.kernel_ref(kind, params, x, y)
    return _frozen(x, y, w, K, dist) + (params,)


def _cov(mellon, kind, params, **kw):
    return getattr(mellon.cov, kind)(*params, **kw)


def _check_inputs(K, dist, d):
    """The conditions on the inputs (checked without a GPU in test_predict_restatement_host.py): few rows carry the
    loose coincident tolerance, many entries are neither negligible nor coincident."""
    co = np.asarray(dist < pr.CO_RADIUS)
    if d == 1:
        assert co.mean() <= 0.05          # one column: every cell has centres within 0.05 by chance -- share of pairs
    else:
        assert co.any(axis=1).mean() <= 0.05
    assert ((np.abs(np.asarray(K, dtype=np.float64)) > 1e-3) & ~co).sum() >= min(10000, K.size // 4)


def _check_rows(got, K, dist, w, mu, label=""):
    """got against mu + K w row by row; returns the bound."""
    mean, absdot = pr.mean_of(K, w, mu)
    bound = pr.row_bound(K, dist, w, absdot, TOLK, TOLCO)
    got = np.asarray(got)
    assert got.shape == (K.shape[0],) and np.all(np.isfinite(got)), label
    err = np.abs(got.astype(LD) - mean).astype(np.float64)
    worst = int(np.argmax(err / bound))
    print(f"{label}: max err {err.max():.3e}, worst row {worst}: err {err[worst]:.3e} bound {bound[worst]:.3e}")
    assert np.all(err <= bound), (label, worst, err[worst], bound[worst], int((err > bound).sum()))
    return bound


# ---- 1. every instantiation of path A ---------------------------------------------------------------------------------
# The issue's four shapes in an order that alternates the parity of ceil(m / 64) (4, 5, 6, 5 tiles): the two d of each
# k-step variant then meet an even and an odd tile count for every kind.
SHAPES_A = [(4096, 256), (4097, 257), (4100, 383), (4223, 320)]
DIMS_A = [1, 32, 33, 52, 53, 64]          # both sides of the KSTEPS boundaries (8 | 13 | 16 k-steps), and d = 1


@pytest.mark.parametrize("kind", ROW_KINDS)
@pytest.mark.parametrize("d", DIMS_A)
def test_row_kernel_every_instantiation(mellon, ctx, kind, d):
    n, m = SHAPES_A[(DIMS_A.index(d) + ROW_KINDS.index(kind)) % 4]
    x, y, w, K, dist, params = _problem(kind, d, n, m, 100 * d + ROW_KINDS.index(kind))
    _check_inputs(K, dist, d)
    got = ctx.predict_mean(_cov(mellon, kind, params).lower(d), x, y, w, MU)
    _check_rows(got, K, dist, w, MU, f"{kind} d={d} n={n} m={m}")


def test_row_kernel_grid_meets_both_tile_parities():
    for ki, kind in enumerate(ROW_KINDS):
        for pair in ((1, 32), (33, 52), (53, 64)):
            tiles = {-(-SHAPES_A[(DIMS_A.index(d) + ki) % 4][1] // 64) % 2 for d in pair}
            assert tiles == {0, 1}, (kind, pair)


# ---- 2. tile and row edges ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [256, 257, 320, 383, 448])  # 4 tiles exact, 5 with one column, 5 exact, 6 ragged, 7 exact
@pytest.mark.parametrize("n", [4096, 4097, 4223])       # exact block count, one row in the last block, one row missing
@pytest.mark.parametrize("kind,d", [("Exponential", 8), ("Matern32", 40), ("RatQuad", 60)])   # 8, 13, 16 k-steps
def test_row_kernel_tile_and_row_edges(mellon, ctx, kind, d, n, m):
    x, y, w, K, dist, params = _problem(kind, d, 4223, 256, 7000 + d, 192)      # one reference; its leading blocks
    x, y, w, K, dist = x[:n], y[:m], w[:m], K[:n, :m], dist[:n, :m]
    _check_inputs(K, dist, d)
    got = ctx.predict_mean(_cov(mellon, kind, params).lower(d), x, y, w, MU)
    _check_rows(got, K, dist, w, MU, f"{kind} d={d} n={n} m={m}")


# ---- 3. column identity -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["Matern52", "RatQuad"])
def test_row_kernel_one_hot_weights_return_the_column(mellon, ctx, kind):
    """w = e_j, mu = 0: the output is column j of K (the other terms are exact zeros), first / last column of a tile,
    of both centre buffers and of all three norm / weight buffers, and the last column of the ragged last tile."""
    n, m, d = 4097, 383, 40
    x, y, _, K, dist, params = _problem(kind, d, n, m, 31 + ROW_KINDS.index(kind))
    _check_inputs(K, dist, d)
    desc = _cov(mellon, kind, params).lower(d)
    tol, _ = pr.pair_tolerance(K, dist, TOLK, TOLCO)
    for j in (0, 63, 64, 127, 128, 191, 192, 320, 382):
        w = np.zeros(m)
        w[j] = 1.0
        got = ctx.predict_mean(desc, x, y, w, 0.0)
        err = np.abs(got.astype(LD) - K[:, j]).astype(np.float64)
        print(f"{kind} column {j}: max err {err.max():.3e}")
        assert np.all(err <= tol[:, j]), (kind, j, err.max())


@pytest.mark.parametrize("kind", ["Matern52", "RatQuad"])
def test_row_kernel_pad_columns_add_nothing(mellon, ctx, kind):
    """w = 1 and a length scale far beyond every distance: K ~ 1 and the output ~ m.  The 65 pad columns of the last
    tile (and two tiles of padding behind it) have k(x, 0) ~ 1 as well: only their zero weights keep them out."""
    n, m, d = 4097, 383, 40
    x, y, _ = pr.make_inputs(n, m, d, 77)
    params = (2.0, 1e9) if kind == "RatQuad" else (1e9,)
    K, dist = pr.kernel_ref(kind, params, x, y)
    w = np.ones(m)
    got = ctx.predict_mean(_cov(mellon, kind, params).lower(d), x, y, w, 0.0)
    assert np.abs(got - m).max() < 1e-3
    _check_rows(got, K, dist, w, 0.0, f"{kind} ls=1e9")


# ---- 4. scratch reuse ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", [("Matern32", 20), ("RatQuad", 60)])
def test_row_kernel_scratch_reuse(mellon, ctx, kind, d):
    """A call with fewer centres after one with more, on one context: the padded copies live in a scratch buffer that is
    reused, so stale centres, norms or weights of the larger call behind row 257 would show in the smaller one."""
    n = 4100
    params = pr.kind_params(kind, d)
    desc = _cov(mellon, kind, params).lower(d)
    xa, ya, wa = pr.make_inputs(n, 383, d, 400 + d)
    xb, yb, wb = pr.make_inputs(n, 257, d, 500 + d)
    first = ctx.predict_mean(desc, xa, ya, wa, MU)
    second = ctx.predict_mean(desc, xb, yb, wb, MU)
    third = ctx.predict_mean(desc, xa, ya, wa, MU)
    Ka, da = pr.kernel_ref(kind, params, xa, ya)
    Kb, db = pr.kernel_ref(kind, params, xb, yb)
    _check_inputs(Ka, da, d)
    _check_inputs(Kb, db, d)
    _check_rows(first, Ka, da, wa, MU, f"{kind} first (m=383)")
    _check_rows(second, Kb, db, wb, MU, f"{kind} second (m=257)")
    _check_rows(third, Ka, da, wa, MU, f"{kind} third (m=383)")
    assert np.array_equal(first, third)


# ---- 5. paths agree where they meet -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ROW_KINDS)
def test_paths_agree_where_they_meet(mellon, ctx, kind):
    """The same 700 rows through the row kernel (as part of 4500), through the MFMA kernel (on their own), and through
    the materialised kernel matrix times a two-column W (a separate branch of mln_predict_mean for mu != 0 and mu == 0;
    RatQuad's kernel matrix has no row kernel, so p = 1 and p = 2 run different kernels)."""
    n, m, d, cut = 4500, 300, 20, 700
    x, y, w, K, dist, params = _problem(kind, d, n, m, 900 + ROW_KINDS.index(kind))
    _check_inputs(K, dist, d)
    desc = _cov(mellon, kind, params).lower(d)
    path_a = ctx.predict_mean(desc, x, y, w, MU)
    bound = _check_rows(path_a, K, dist, w, MU, f"{kind} path A")
    path_c = ctx.predict_mean(desc, np.ascontiguousarray(x[:cut]), y, w, MU)
    _check_rows(path_c, K[:cut], dist[:cut], w, MU, f"{kind} path C")
    assert np.all(np.abs(path_a[:cut] - path_c) <= 2 * bound[:cut])
    w2 = np.random.default_rng(5).normal(size=m)
    W = np.column_stack([w, w2])
    for mu in (MU, 0.0):
        both = ctx.predict_mean(desc, x, y, W, mu)
        assert both.shape == (n, 2)
        b0 = _check_rows(both[:, 0], K, dist, w, mu, f"{kind} p=2 mu={mu} column 0")
        _check_rows(both[:, 1], K, dist, w2, mu, f"{kind} p=2 mu={mu} column 1")
        if mu == MU:
            assert np.all(np.abs(both[:, 0] - path_a) <= 2 * b0)


# ---- 6. path C beyond the row kernels -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", pr.KINDS)
@pytest.mark.parametrize("n,m,d", [(300, 130, 65), (300, 130, 67), (300, 130, 130),    # wider than any row kernel
                                   (64, 64, 3),                                         # n m = 4096 exactly: still C
                                   (63, 65, 3)])                                        # just below: path D
def test_mfma_kernel_wide_and_small(mellon, ctx, kind, n, m, d):
    x, y, w = pr.make_inputs(n, m, d, 10 * d + n + pr.KINDS.index(kind))
    params = pr.kind_params(kind, d)
    K, dist = pr.kernel_ref(kind, params, x, y)
    _check_inputs(K, dist, d)
    got = ctx.predict_mean(_cov(mellon, kind, params).lower(d), x, y, w, MU)
    _check_rows(got, K, dist, w, MU, f"{kind} d={d} n={n} m={m}")


# ---- 7. paths D and E ---------------------------------------------------------------------------------------------------
def _programs(mellon, x, y, xt, yt):
    """(name, covariance, longdouble K, distances that define co, cells, centres) for single leaves over column subsets
    and composite programs of two leaves over disjoint column sets, d = 6."""
    cov = mellon.cov
    mask = np.array([True, False, True, False, False, True])
    Ka, da = pr.kernel_ref("Matern52", (1.7,), x, y, [0, 1, 2])
    Kb, db = pr.kernel_ref("Exponential", (1.3,), x, y, [3, 4, 5])
    a, b = cov.Matern52(1.7, active_dims=[0, 1, 2]), cov.Exponential(1.3, active_dims=[3, 4, 5])
    Ke, de = pr.kernel_ref("ExpQuad", (1.7,), x, y, [0, 2, 5])
    Km, dm = pr.kernel_ref("Matern32", (1.1,), x, y, mask)
    Ks, ds = pr.kernel_ref("Matern52", (2.1,), xt, yt, slice(None, -1))
    Kt, _ = pr.kernel_ref("ExpQuad", (1.7,), xt, yt, -1)
    return [
        ("index list", cov.ExpQuad(1.7, active_dims=[0, 2, 5]), Ke, de, x, y),
        ("boolean mask", cov.Matern32(1.1, active_dims=mask), Km, dm, x, y),
        ("a * b", a * b, Ka * Kb, np.minimum(da, db), x, y),
        ("a + b", a + b, Ka + Kb, np.minimum(da, db), x, y),
        ("a + 2.0", a + 2.0, Ka + 2, da, x, y),
        ("3.0 * a", 3.0 * a, 3 * Ka, da, x, y),
        # state leaf x time leaf of different kinds: not the product row kernel's.  The time column holds small integers,
        # whose squared distance is exact in any arithmetic: only the state leaf's distance defines co
        ("Matern52(:-1) * ExpQuad(-1)", cov.Matern52(2.1, active_dims=slice(None, -1)) * cov.ExpQuad(1.7, active_dims=-1),
         Ks * Kt, ds, xt, yt),
    ]


@functools.lru_cache(maxsize=2)
def _program_inputs(n, m):
    """The recipe at d = 6, and a copy whose last column holds time points 0..5."""
    x, y, w = pr.make_inputs(n, m, 6, n + m)
    rng = np.random.default_rng(n)
    xt, yt = x.copy(), y.copy()
    xt[:, -1], yt[:, -1] = rng.integers(0, 6, size=n), rng.integers(0, 6, size=m)
    return _frozen(x, y, w, xt, yt)


@pytest.mark.parametrize("n,m", [(4100, 257), (130, 67)])
@pytest.mark.parametrize("which", range(7))
def test_tiled_kernels_subsets_and_composites(mellon, ctx, n, m, which):
    x, y, w, xt, yt = _program_inputs(n, m)
    name, c, K, dist, xs, ys = _programs(mellon, x, y, xt, yt)[which]
    _check_inputs(K, dist, 6)
    got = ctx.predict_mean(c.lower(6), xs, ys, w, MU)
    _check_rows(got, K, dist, w, MU, f"{name} n={n} m={m}")


# ---- 8. resident arrays -------------------------------------------------------------------------------------------------
def test_resident_arrays_and_repeatability(mellon, ctx):
    n, m, d = 4097, 257, 33
    x, y, w, K, dist, params = _problem("Matern52", d, n, m, 8)
    desc = _cov(mellon, "Matern52", params).lower(d)
    host = ctx.predict_mean(desc, x, y, w, MU)
    _check_rows(host, K, dist, w, MU, "host arrays")
    assert np.array_equal(host, ctx.predict_mean(desc, x, y, w, MU))
    out = ctx.empty((n,))
    res = ctx.predict_mean(desc, ctx.to_device(x), ctx.to_device(y), w, MU, out=out)
    assert res is out
    assert np.array_equal(out.to_host(), host)
    res = ctx.predict_mean(desc, ctx.to_device(x), ctx.to_device(y), ctx.to_device(w), MU, out=out)
    assert res is out and np.array_equal(out.to_host(), host)
