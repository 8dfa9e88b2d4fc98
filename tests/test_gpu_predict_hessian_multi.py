"""mln_predict_hessian_multi and mln_predict_hessian_logdet: the Hessians of a p-output predictive mean in one device call, and
their sign / log|det| without the Hessians leaving the device -- against the single-output call column by column (itself pinned
to the oracle by test_predict_hessian_matches_oracle), on every route: p == 1, the per-column route below 2^16 pairs, the batched
route (ragged tiles, output blocks, the row-chunk seam, a Linear factor), and through Predictor / ExpPredictor / PredictorTime
and the time grid.

Bound on the batched route: max|H - H_single| < 1e-10 max|H_single|, the bound test_predictors_with_p_outputs uses for Hessians
column against single -- the two differ only in whether w_j multiplies the coefficient or the centre operand, one rounding per
term over m <= 257 terms of the same expansion.  Bound on logabsdet: that of tests/test_gpu_slogdet.py,
err <= 4 max_batch(err_LAPACK) + k^2 2^-52 against the longdouble LU of the same matrices."""
import functools

import numpy as np
import pytest

import slogdet_reference as sr
from oracle import mellon_oracle as mo
from test_gpu_predict_gradient_multi import _pair, _trees

pytestmark = pytest.mark.gpu

BATCHED_MIN_PAIRS = 1 << 16
SEAM = 16384                     # rows per chunk of both Hessian launchers at these sizes


@pytest.fixture(scope="module")
def ctx():
    from mellon_amd import _lib
    return _lib.default_context()


def _err(a, ref):
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300)


@functools.lru_cache(maxsize=None)
def _inputs(n, m, d, p):
    rng = np.random.default_rng(2000 * n + 10 * m + d + p)
    xq, c, W = rng.normal(size=(n, d)), rng.normal(size=(m, d)), rng.normal(size=(m, p))
    for a in (xq, c, W):
        a.flags.writeable = False
    return xq, c, W


_SINGLES = {}


def _singles(ctx, name, n, m, d, p):
    """The single-output Hessians (n, p, d, d) of one tree: computed once, shared read-only."""
    key = (name, n, m, d, p)
    if key not in _SINGLES:
        xq, c, W = _inputs(n, m, d, p)
        desc = _trees(d)[name].lower(d)
        H = np.stack([ctx.predict_hessian(desc, xq, c, np.ascontiguousarray(W[:, q])) for q in range(p)], axis=1)
        H.flags.writeable = False
        _SINGLES[key] = H
    return _SINGLES[key]


def _ncol_max(k, d):
    nd = [len(leaf[3]) for leaf in k.lower(d).leaves]
    return max(a * b + a + b + 1 for i, a in enumerate(nd) for b in nd[i:])


def _check_logdet(A, sign, logabs, what):
    """Item 5's bound for device results (sign, logabs) of the matrices A; prints the figures."""
    A = A.reshape((-1,) + A.shape[-2:])
    s_ref = sr.slogdet_longdouble(A)[0]
    assert np.array_equal(np.asarray(sign).reshape(-1), s_ref), what
    e_dev, e_lap, bound = sr.logdet_errors(A, logabs)
    print(f"{what}: device {e_dev:.2e}, LAPACK {e_lap:.2e}, bound {bound:.2e}")
    assert e_dev <= bound, what


def test_the_entries_exist(ctx):
    for name in ("mln_predict_hessian_multi", "mln_slogdet_batched", "mln_predict_hessian_logdet"):
        assert hasattr(ctx.lib, name)
    xq, c, W = _inputs(20, 30, 3, 4)
    assert ctx.predict_hessian(_trees(3)["leaf"].lower(3), xq, c, W).shape == (20, 4, 3, 3)


SHAPES = [(1, 1, 1, 1), (20, 30, 3, 4), (300, 257, 5, 3), (SEAM + 37, 64, 2, 2)]


@pytest.mark.parametrize("n,m,d,p", SHAPES)
def test_matches_the_single_output_call(ctx, n, m, d, p):
    xq, c, W = _inputs(n, m, d, p)
    for name, k in _trees(d).items():
        desc = k.lower(d)
        H, ref = ctx.predict_hessian(desc, xq, c, W), _singles(ctx, name, n, m, d, p)
        assert H.shape == (n, p, d, d)
        assert np.array_equal(H, ctx.predict_hessian(desc, xq, c, W)), name               # two calls, identical bits
        assert np.abs(H - np.swapaxes(H, 2, 3)).max() <= 1e-12 * max(np.abs(H).max(), 1e-300), name
        if n * m >= BATCHED_MIN_PAIRS and p > 1:
            e = _err(H, ref)
            print(f"({n}, {m}, {d}, {p}) {name}: {e:.2e}")
            assert e < 1e-10, name
        else:                                           # p == 1, fewer than 2^16 pairs: the single-output call, bit for bit
            assert np.array_equal(H, ref), name


def test_one_tree_against_the_oracle(ctx):
    """(20, 30, 3, 4), the composite tree, at test_predict_hessian_matches_oracle's tolerance for its kernels."""
    n, m, d, p = 20, 30, 3, 4
    xq, c, W = _inputs(n, m, d, p)
    k = _trees(d)["composite"]
    H = ctx.predict_hessian(k.lower(d), xq, c, W)
    for q in range(p):
        ref = mo.Predictor(_pair(k), c, np.ascontiguousarray(W[:, q]), 0.0, m).hessian(xq)
        assert np.abs(H[:, q] - ref).max() < 2e-7 * np.abs(ref).max()


def test_output_blocks_two_full_and_a_ragged_one(ctx, monkeypatch):
    """p = 7 in blocks of P_b = 3 (the column budget is 3 ncol_max of each tree) and of P_b = 1 (a budget of 1)."""
    n, m, d, p = 300, 257, 5, 7
    xq, c, W = _inputs(n, m, d, p)
    for name, k in _trees(d).items():
        desc, ref = k.lower(d), _singles(ctx, name, n, m, d, p)
        monkeypatch.delenv("MELLON_AMD_HESS_COLS", raising=False)
        whole = ctx.predict_hessian(desc, xq, c, W)
        monkeypatch.setenv("MELLON_AMD_HESS_COLS", str(3 * _ncol_max(k, d) + 1))
        H3 = ctx.predict_hessian(desc, xq, c, W)
        monkeypatch.setenv("MELLON_AMD_HESS_COLS", "1")
        H1 = ctx.predict_hessian(desc, xq, c, W)
        print(f"{name}: one block {_err(whole, ref):.2e}, P_b = 3 {_err(H3, ref):.2e} (to one block {_err(H3, whole):.2e}), "
              f"P_b = 1 {_err(H1, ref):.2e} (to one block {_err(H1, whole):.2e})")
        assert _err(whole, ref) < 1e-10 and _err(H3, ref) < 1e-10 and _err(H1, ref) < 1e-10, name


@pytest.mark.parametrize("n,m", [(20, 30), (300, 257)])
def test_a_zero_column_and_inactive_dims_are_exact_zeros(ctx, n, m):
    from mellon_amd import cov
    d, p = 5, 3
    rng = np.random.default_rng(n + m)
    xq, c, W = rng.normal(size=(n, d)), rng.normal(size=(m, d)), rng.normal(size=(m, p))
    W[:, 1] = 0.0
    trees = [cov.Matern52(1.5, active_dims=[1, 3]),
             cov.Matern52(1.5, active_dims=[0, 2]) * cov.ExpQuad(1.0, active_dims=[2, 3])]
    x_dev = ctx.to_device(xq)
    for k, inactive in zip(trees, ([0, 2, 4], [1, 4])):
        H = ctx.predict_hessian(k.lower(d), xq, c, W)
        assert not H[:, 1].any()
        assert not H[:, :, inactive, :].any() and not H[:, :, :, inactive].any()
        active = [i for i in range(d) if i not in inactive]
        assert np.all(np.abs(H[:, [0, 2]][:, :, active][:, :, :, active]).max(axis=0) > 0)
        ref = np.stack([ctx.predict_hessian(k.lower(d), xq, c, np.ascontiguousarray(W[:, q])) for q in range(p)], axis=1)
        assert _err(H, ref) < 1e-10
        assert np.array_equal(ctx.predict_hessian(k.lower(d), x_dev, c, W), H)           # device-resident queries: same bits
        sign, logabs = ctx.predict_hessian_logdet(k.lower(d), xq, c, W)
        assert np.array_equal(sign, np.zeros((n, p))) and np.all(logabs == -np.inf)      # inactive dims: singular everywhere
    x_dev.free()


@pytest.mark.parametrize("n,m,d,p", [(300, 257, 5, 3), (SEAM + 37, 64, 2, 2)])
def test_fused_logdet_factors_the_bits_predict_hessian_returns(ctx, n, m, d, p):
    xq, c, W = _inputs(n, m, d, p)
    W0 = np.array(W)
    W0[:, 1] = 0.0                                       # a zero column: (0, -inf) for that output
    for name, k in _trees(d).items():
        desc = k.lower(d)
        H = ctx.predict_hessian(desc, xq, c, W)
        for lead in sorted({d, max(d - 1, 1)}):
            sign, logabs = ctx.predict_hessian_logdet(desc, xq, c, W, lead=lead)
            assert sign.shape == logabs.shape == (n, p)
            s2, l2 = ctx.slogdet_batched(H, lead=lead)
            assert np.array_equal(sign, s2), (name, lead)
            sub = np.ascontiguousarray(H[..., :lead, :lead])
            _check_logdet(sub, sign, logabs, f"({n}, {m}, {d}, {p}) {name} lead {lead} fused")
            _check_logdet(sub, s2, l2, f"({n}, {m}, {d}, {p}) {name} lead {lead} slogdet_batched")
            print(f"    fused equals slogdet_batched(predict_hessian): {np.array_equal(logabs, l2)}")
        # (the Hessian of the `linear` tree lives on dims [0, 2] alone: singular everywhere, (0, -inf) from both)
        s0, l0 = ctx.predict_hessian_logdet(desc, xq, c, W0)
        assert np.array_equal(s0[:, 1], np.zeros(n)) and np.all(l0[:, 1] == -np.inf), name
        keep = [q for q in range(p) if q != 1]           # the other outputs do not notice
        assert np.array_equal(s0[:, keep], sign[:, keep]) and np.array_equal(l0[:, keep], logabs[:, keep]), name
        assert name == "linear" or (np.all(s0[:, 0] != 0) and np.all(np.isfinite(l0[:, 0]))), name


def test_fused_logdet_single_output_and_small_routes(ctx):
    """p == 1 above the threshold and p = 4 below it go through the single-output launcher: still the bits of predict_hessian."""
    for (n, m, d, p), W_of in (((300, 257, 5, 3), lambda W: np.ascontiguousarray(W[:, 0])), ((20, 30, 3, 4), lambda W: W)):
        xq, c, W = _inputs(n, m, d, p)
        w = W_of(W)
        for name, k in _trees(d).items():
            H = ctx.predict_hessian(k.lower(d), xq, c, w)
            sign, logabs = ctx.predict_hessian_logdet(k.lower(d), xq, c, w)
            assert sign.shape == H.shape[:-2]
            s2, l2 = ctx.slogdet_batched(H)
            assert np.array_equal(sign, s2) and np.array_equal(logabs, l2), name
            _check_logdet(H, sign, logabs, f"({n}, {m}, {d}) {name} p = {1 if w.ndim == 1 else p}")


def test_bad_shapes_are_refused(ctx):
    from mellon_amd import base_cov, cov
    desc = cov.Matern52(1.0).lower(3)
    x, c, W = np.zeros((4, 3)), np.zeros((5, 3)), np.zeros((5, 2))
    with pytest.raises(ValueError):
        ctx.predict_hessian(desc, x, c, np.zeros((4, 2)))                   # rows of W are centres
    with pytest.raises(ValueError):
        ctx.predict_hessian(desc, x, c, np.zeros((5, 2, 2)))
    out = np.empty(4 * 2 * 9)
    assert ctx.lib.mln_predict_hessian_multi(ctx.handle, desc.ref, x.ctypes.data, 4, 3, c.ctypes.data, 5, W.ctypes.data, 0,
                                             out.ctypes.data) != 0          # p < 1
    value_only = base_cov.LoweredCov([(7, 1.0, 1.0, np.arange(3))], [(0, 0, 0.0)])
    with pytest.raises(Exception):                                          # a value-only leaf has no derivatives
        ctx.predict_hessian(value_only, x, c, W)
    with pytest.raises(Exception):
        ctx.predict_hessian_logdet(value_only, x, c, W)
    with pytest.raises(Exception):
        ctx.predict_hessian_logdet(desc, x, c, W, lead=4)                   # lead > d
    with pytest.raises(NotImplementedError):
        ctx.predict_hessian_logdet(cov.Matern52(9.0).lower(65), np.zeros((2, 65)), np.zeros((3, 65)), np.zeros(3))
    assert ctx.predict_hessian(desc, np.zeros((0, 3)), c, W).shape == (0, 2, 3, 3)


@pytest.mark.parametrize("n,m", [(20, 30), (300, 257)])
def test_predictors_with_p_outputs(ctx, n, m):
    """Predictor, ExpPredictor and PredictorTime with (m, p) weights: `hessian` column by column the single-output predictor's."""
    from mellon_amd import cov
    from mellon_amd.base_predictor import ExpPredictor, Predictor, PredictorTime
    d, p = 4, 3
    rng = np.random.default_rng(7 * n + m)
    xq, c, W = rng.normal(size=(n, d)), rng.normal(size=(m, d)), rng.normal(size=(m, p)) * 0.1
    plain = cov.Matern52(2.5)
    timed = cov.Matern52(2.0, active_dims=slice(None, -1)) * cov.Matern52(1.3, active_dims=-1)

    def columns(make, *args):
        return np.stack([make(np.ascontiguousarray(W[:, q])).hessian(*args) for q in range(p)], axis=1)

    for cls in (Predictor, ExpPredictor):
        H = cls(plain, c, W, 0.3).hessian(xq)
        assert H.shape == (n, p, d, d)
        e = _err(H, columns(lambda w: cls(plain, c, w, 0.3), xq))
        print(f"{cls.__name__} ({n}, {m}): {e:.2e}")
        assert e < 1e-10
    H = PredictorTime(timed, c, W, 0.3).hessian(xq[:, :-1], time=0.4)
    assert H.shape == (n, p, d - 1, d - 1)
    e = _err(H, columns(lambda w: PredictorTime(timed, c, w, 0.3), xq[:, :-1], 0.4))
    print(f"PredictorTime ({n}, {m}): {e:.2e}")
    assert e < 1e-10


def test_predictor_log_determinant_routes(ctx, monkeypatch):
    from mellon_amd import _lib, cov
    from mellon_amd.base_predictor import ExpPredictor, Predictor
    calls = []
    fused = _lib.Context.predict_hessian_logdet
    monkeypatch.setattr(_lib.Context, "predict_hessian_logdet", lambda self, *a, **k: calls.append(1) or fused(self, *a, **k))
    d = 4
    for n, m in ((300, 257), (20, 30)):
        rng = np.random.default_rng(n + 3 * m)
        xq, c, w = rng.normal(size=(n, d)), rng.normal(size=(m, d)), rng.normal(size=m) * 0.1
        pred = Predictor(cov.Matern52(2.5), c, w, 0.3)
        del calls[:]
        sign, logabs = pred.hessian_log_determinant(xq)
        H = pred.hessian(xq)
        s_np, l_np = np.linalg.slogdet(H)
        if n * m >= BATCHED_MIN_PAIRS:                  # above the threshold: the fused entry
            assert calls
            assert np.array_equal(sign, s_np)
            _check_logdet(H, sign, logabs, f"Predictor ({n}, {m})")
        else:                                           # below it: the host path, its bits
            assert not calls
            assert np.array_equal(sign, s_np) and np.array_equal(logabs, l_np)
        ep = ExpPredictor(cov.Matern52(2.5), c, w, 0.3)
        del calls[:]
        sign, logabs = ep.hessian_log_determinant(xq)
        s_np, l_np = np.linalg.slogdet(ep.hessian(xq))
        assert not calls and np.array_equal(sign, s_np) and np.array_equal(logabs, l_np)


def test_time_grid(ctx, monkeypatch):
    """Matern52(state) * ExpQuad(time), n = 300, m = 257, d = 4 + time, T = 5: the grid is one T-output call of the state kernel.

    Measured on an MI355X: grid Hessians against the loop 2.0e-15 of their maximum; log-determinants, each side against the
    longdouble LU of the Hessians it factored: grid 8.7e-13, loop 1.2e-12 (bound 5.0e-12), LAPACK on the grid's 7.5e-13.  The
    two results themselves differ by 4.60e-11 -- and the longdouble log-determinants of the two sets of Hessians by 4.64e-11:
    the largest condition number among the 1 500 Hessians is 1.1e5, so last-bit differences of the inputs are worth that much
    before either side rounds anything.  No bound on rounding in the factorisation can cover a difference of the inputs, which
    is why the loop enters the bound through its own error, not through its values."""
    from mellon_amd import _lib, cov
    from mellon_amd.base_predictor import PredictorTime
    n, m, d, T = 300, 257, 5, 5
    rng = np.random.default_rng(11)
    xs, c, w = rng.normal(size=(n, d - 1)), rng.normal(size=(m, d)), rng.normal(size=m) * 0.1
    ts = np.linspace(-0.8, 1.1, T)
    tree = cov.Matern52(2.0, active_dims=slice(None, -1)) * cov.ExpQuad(1.2, active_dims=-1)
    pt = PredictorTime(tree, c, w, 0.3)
    seen = {"hessian": [], "logdet": []}
    hess, fused = _lib.Context.predict_hessian, _lib.Context.predict_hessian_logdet
    monkeypatch.setattr(_lib.Context, "predict_hessian",
                        lambda self, desc, x, cc, W: seen["hessian"].append(np.shape(W)) or hess(self, desc, x, cc, W))
    monkeypatch.setattr(_lib.Context, "predict_hessian_logdet",
                        lambda self, desc, x, cc, W, lead=None: seen["logdet"].append((np.shape(W), lead))
                        or fused(self, desc, x, cc, W, lead=lead))

    def reset():
        del seen["hessian"][:], seen["logdet"][:]

    H = pt.hessian(xs, multi_time=ts)
    assert H.shape == (n, T, d - 1, d - 1) and seen["hessian"] == [(m, T)]
    loop = np.stack([pt.hessian(xs, time=float(t)) for t in ts], axis=1)
    e = _err(H, loop)
    print(f"grid Hessian against the per-time loop: {e:.2e}")
    assert e < 1e-10
    reset()
    sign, logabs = pt.hessian_log_determinant(xs, multi_time=ts)
    assert sign.shape == logabs.shape == (n, T) and seen["logdet"] == [((m, T), d - 1)] and not seen["hessian"]
    pairs = [pt.hessian_log_determinant(xs, time=float(t)) for t in ts]
    s_loop, l_loop = (np.stack([pr[k] for pr in pairs], axis=1) for k in (0, 1))
    assert np.array_equal(sign, s_loop)
    _check_logdet(H, sign, logabs, "grid log-determinant, its own Hessians")           # LAPACK as the yardstick
    # ... and the loop as the yardstick, as numpy's slogdet is for Predictor above: the error of the grid's values against the
    # longdouble LU of the Hessians the grid factors, within 4 max(the loop's error against the longdouble LU of the Hessians the
    # loop factors) + k^2 2^-52.  The raw difference of the two results is printed, not bounded: the two factor Hessians that
    # differ in their last bits (e above), which a Hessian of condition number kappa turns into kappa e of log|det| before any
    # factorisation rounds -- the difference of the two longdouble values, printed next to it, is that part.
    ref_grid, ref_loop = (sr.slogdet_longdouble(A.reshape(-1, d - 1, d - 1))[1].reshape(n, T) for A in (H, loop))
    e_grid, e_loop = float(np.abs(logabs - ref_grid).max()), float(np.abs(l_loop - ref_loop).max())
    bound = 4.0 * e_loop + (d - 1) ** 2 * sr.EPS
    print(f"grid error {e_grid:.2e}, loop error {e_loop:.2e}, bound {bound:.2e}; raw grid - loop {np.abs(logabs - l_loop).max():.2e}, "
          f"of which the inputs' own difference {float(np.abs(ref_grid - ref_loop).max()):.2e}, largest condition number "
          f"{np.linalg.cond(loop).max():.1e}")
    assert e_grid <= bound
    # what takes the loop: T = 1, 2-D weights, a tree that is no state x time product
    reset()
    assert pt.hessian(xs, multi_time=ts[:1]).shape == (n, 1, d - 1, d - 1) and seen["hessian"] == [(m,)]
    reset()
    W2 = np.ascontiguousarray(np.stack([w, 2 * w], axis=1))
    assert PredictorTime(tree, c, W2, 0.3).hessian(xs, multi_time=ts[:2]).shape == (n, 2, 2, d - 1, d - 1)
    assert seen["hessian"] == [(m, 2), (m, 2)]
    reset()
    summed = PredictorTime(cov.Matern52(2.0, active_dims=slice(None, -1)) + cov.ExpQuad(1.2, active_dims=-1), c, w, 0.3)
    s, _ = summed.hessian_log_determinant(xs, multi_time=ts[:2])
    assert s.shape == (n, 2) and seen["logdet"] == [((m,), d - 1)] * 2
