"""mln_predict_gradient_multi: the gradient of a p-output predictive mean in one device call, against the oracle's k_grad
contracted with the weights -- every route (p == 1, the batched GEMM route for stationary leaves above 2^16 pairs, the
per-column route below it and for a Linear leaf), ragged tiles, output blocks and the row-chunk seam.

Bound: that of test_predict_gradient_matches_contracted_k_grad, max|g - ref| < 1e-10 max|ref| (the oracle's k_grad divides by
dist + 1e-12 where the device divides by dist: 1e-12 relative at the O(1) distances of normal inputs; the rest is fp64
summation over m <= 257 terms)."""
import functools

import numpy as np
import pytest

from oracle import mellon_oracle as mo

pytestmark = pytest.mark.gpu

BATCHED_MIN_PAIRS = 1 << 16


@pytest.fixture(scope="module")
def ctx():
    from mellon_amd import _lib
    return _lib.default_context()


def _pair(product_cov):
    return mo.Covariance.from_dict(product_cov.to_dict())


def _trees(d):
    """name -> covariance; the trees that need three columns appear from d = 3 on, the product ones from d = 2."""
    from mellon_amd import cov
    s = np.sqrt(d)
    trees = {"leaf": cov.Matern52(1.7 * s)}
    if d >= 2:
        trees["product"] = cov.Matern52(1.5 * s, active_dims=slice(None, -1)) * cov.ExpQuad(1.2, active_dims=-1)
        trees["composite"] = (cov.Matern52(2.0 * s) * cov.RatQuad(1.5, 3.0 * s)) ** 2.0
    if d >= 3:
        trees["linear"] = cov.Matern32(2.0, active_dims=[0, 2]) + 0.5 * cov.Linear(3.0)
    return trees


@functools.lru_cache(maxsize=None)
def _case(n, m, d, p):
    """Inputs and, per tree, the oracle gradient (n, p, d); computed once, shared read-only."""
    rng = np.random.default_rng(1000 * n + 10 * m + d + p)
    xq, c, W = rng.normal(size=(n, d)), rng.normal(size=(m, d)), rng.normal(size=(m, p))
    refs = {name: np.einsum("jq,jik->iqk", W, _pair(k).k_grad(c)(xq)) for name, k in _trees(d).items()}
    for a in (xq, c, W, *refs.values()):
        a.flags.writeable = False
    return xq, c, W, refs


def _err(g, ref):
    return np.abs(g - ref).max() / max(np.abs(ref).max(), 1e-300)


def _singles(ctx, desc, xq, c, W):
    return np.stack([ctx.predict_gradient(desc, xq, c, np.ascontiguousarray(W[:, q])) for q in range(W.shape[1])], axis=1)


def test_the_entry_exists(ctx):
    assert hasattr(ctx.lib, "mln_predict_gradient_multi")


SHAPES = [(1, 1, 1, 1), (20, 30, 3, 4), (300, 257, 5, 3), (32768 + 37, 64, 2, 2)]


@pytest.mark.parametrize("n,m,d,p", SHAPES)
def test_matches_the_contracted_k_grad(ctx, n, m, d, p):
    xq, c, W, refs = _case(n, m, d, p)
    for name, k in _trees(d).items():
        g = ctx.predict_gradient(k.lower(d), xq, c, W)
        assert g.shape == (n, p, d)
        e = _err(g, refs[name])
        print(f"({n}, {m}, {d}, {p}) {name}: {e:.2e}")
        assert e < 1e-10, name
        assert np.array_equal(g, ctx.predict_gradient(k.lower(d), xq, c, W)), name       # two calls, identical bits
        batched = name != "linear" and n * m >= BATCHED_MIN_PAIRS and p > 1
        if not batched:
            # p == 1, fewer than 2^16 pairs, a Linear leaf: the single-output routes, bit for bit
            assert np.array_equal(g, _singles(ctx, k.lower(d), xq, c, W)), name


def test_output_blocks_two_full_and_a_ragged_one(ctx, monkeypatch):
    """p = 7 in blocks of P_b = 3: the column budget 18 holds three outputs of nd + 1 = 6 columns (five for the state leaf of
    the product tree);
    the difference to one block of 7 is printed."""
    n, m, d, p = 300, 257, 5, 7
    xq, c, W, refs = _case(n, m, d, p)
    for name, k in _trees(d).items():
        monkeypatch.delenv("MELLON_AMD_GRAD_COLS", raising=False)
        whole = ctx.predict_gradient(k.lower(d), xq, c, W)
        monkeypatch.setenv("MELLON_AMD_GRAD_COLS", "18")
        g = ctx.predict_gradient(k.lower(d), xq, c, W)
        e = _err(g, refs[name])
        print(f"P_b = 3, {name}: {e:.2e}; against one block {_err(g, whole):.2e}")
        assert e < 1e-10 and _err(whole, refs[name]) < 1e-10, name
        monkeypatch.setenv("MELLON_AMD_GRAD_COLS", "1")                 # below nd + 1: one output per block
        assert _err(ctx.predict_gradient(k.lower(d), xq, c, W), refs[name]) < 1e-10, name


@pytest.mark.parametrize("n,m", [(20, 30), (300, 257)])
def test_a_zero_column_and_inactive_dims_are_exact_zeros(ctx, n, m):
    from mellon_amd import cov
    d, p = 5, 3
    rng = np.random.default_rng(n + m)
    xq, c, W = rng.normal(size=(n, d)), rng.normal(size=(m, d)), rng.normal(size=(m, p))
    W[:, 1] = 0.0
    trees = [cov.Matern52(1.5, active_dims=[1, 3]),
             cov.Matern52(1.5, active_dims=[0, 2]) * cov.ExpQuad(1.0, active_dims=[2, 3])]
    for k, inactive in zip(trees, ([0, 2, 4], [1, 4])):
        g = ctx.predict_gradient(k.lower(d), xq, c, W)
        assert not g[:, 1].any()
        assert not g[:, :, inactive].any()
        active = [i for i in range(d) if i not in inactive]
        assert np.all(np.abs(g[:, [0, 2]][:, :, active]).max(axis=0) > 0)
        ref = np.einsum("jq,jik->iqk", W, _pair(k).k_grad(c)(xq))
        assert _err(g, ref) < 1e-10


@pytest.mark.parametrize("n,m", [(20, 30), (300, 257)])
def test_device_queries_and_p_equal_one(ctx, n, m):
    xq, c, W, _ = _case(300, 257, 5, 3) if (n, m) == (300, 257) else _case(20, 30, 3, 4)
    d = xq.shape[1]
    x_dev = ctx.to_device(xq)
    for name, k in _trees(d).items():
        desc = k.lower(d)
        assert np.array_equal(ctx.predict_gradient(desc, x_dev, c, W), ctx.predict_gradient(desc, xq, c, W)), name
        # p == 1 through the new entry is mln_predict_gradient
        one = ctx.predict_gradient(desc, xq, c, np.ascontiguousarray(W[:, :1]))
        assert one.shape == (n, 1, d)
        assert np.array_equal(one[:, 0], ctx.predict_gradient(desc, xq, c, np.ascontiguousarray(W[:, 0]))), name
    x_dev.free()


def test_bad_shapes_are_refused(ctx):
    from mellon_amd import cov
    desc = cov.Matern52(1.0).lower(3)
    x, c = np.zeros((4, 3)), np.zeros((5, 3))
    with pytest.raises(ValueError):
        ctx.predict_gradient(desc, x, c, np.zeros((4, 2)))              # rows of W are centres
    with pytest.raises(ValueError):
        ctx.predict_gradient(desc, x, c, np.zeros((5, 2, 2)))
    out = np.empty(4 * 3)
    W = np.zeros((5, 2))
    rc = ctx.lib.mln_predict_gradient_multi(ctx.handle, desc.ref, x.ctypes.data, 4, 3, c.ctypes.data, 5, W.ctypes.data, 0,
                                            out.ctypes.data)
    assert rc != 0                                                       # p < 1
    with pytest.raises(Exception):                                       # a value-only leaf has no derivatives
        ctx.predict_gradient(__import__("mellon_amd").base_cov.LoweredCov([(7, 1.0, 1.0, np.arange(3))], [(0, 0, 0.0)]),
                             x, c, W)
    assert ctx.predict_gradient(desc, np.zeros((0, 3)), c, W).shape == (0, 2, 3)


@pytest.mark.parametrize("n,m", [(20, 30), (300, 257)])
def test_predictors_with_p_outputs(ctx, n, m):
    """Predictor, ExpPredictor and PredictorTime built directly with (m, p) weights: (n, p, d), (n, p, d) and (n, p, d - 1),
    column by column the single-output predictor's result."""
    from mellon_amd import cov
    from mellon_amd.base_predictor import ExpPredictor, Predictor, PredictorTime
    d, p = 4, 3
    rng = np.random.default_rng(7 * n + m)
    xq, c, W = rng.normal(size=(n, d)), rng.normal(size=(m, d)), rng.normal(size=(m, p)) * 0.1
    plain = cov.Matern52(2.5)
    timed = cov.Matern52(2.0, active_dims=slice(None, -1)) * cov.Matern52(1.3, active_dims=-1)

    def columns(make, method, *args):
        return np.stack([getattr(make(np.ascontiguousarray(W[:, q])), method)(*args) for q in range(p)], axis=1)

    g = Predictor(plain, c, W, 0.3).gradient(xq)
    assert g.shape == (n, p, d)
    assert _err(g, columns(lambda w: Predictor(plain, c, w, 0.3), "gradient", xq)) < 1e-10
    g = ExpPredictor(plain, c, W, 0.3).gradient(xq)
    assert g.shape == (n, p, d)
    assert _err(g, columns(lambda w: ExpPredictor(plain, c, w, 0.3), "gradient", xq)) < 1e-10
    H = ExpPredictor(plain, c, W, 0.3).hessian(xq)
    assert H.shape == (n, p, d, d)
    assert _err(H, columns(lambda w: ExpPredictor(plain, c, w, 0.3), "hessian", xq)) < 1e-10
    pt = PredictorTime(timed, c, W, 0.3)
    one = lambda w: PredictorTime(timed, c, w, 0.3)                      # noqa: E731
    g = pt.gradient(xq[:, :-1], time=0.4)
    assert g.shape == (n, p, d - 1)
    assert _err(g, columns(one, "gradient", xq[:, :-1], 0.4)) < 1e-10
    td = pt.time_derivative(xq[:, :-1], time=0.4)
    assert td.shape == (n, p)
    assert _err(td, columns(one, "time_derivative", xq[:, :-1], 0.4)) < 1e-10
    H = pt.hessian(xq[:, :-1], time=0.4)
    assert H.shape == (n, p, d - 1, d - 1)
    assert _err(H, columns(one, "hessian", xq[:, :-1], 0.4)) < 1e-10
    sign, logdet = pt.hessian_log_determinant(xq[:, :-1], time=0.4)
    assert sign.shape == (n, p) and logdet.shape == (n, p)
    # 2-D weights and multi_time: the per-time loop, (n, T, p, d - 1)
    gm = pt.gradient(xq[:, :-1], multi_time=[0.4, 0.9])
    assert gm.shape == (n, 2, p, d - 1) and np.array_equal(gm[:, 0], g)
