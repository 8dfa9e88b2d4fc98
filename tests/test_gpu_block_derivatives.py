"""Gradient / Hessian of the predictive mean and Covariance.k_grad for covariance trees that are not one device program
(mellon_amd/block_derivatives.py + csrc/cov_block_deriv.hip), on a real MI355X (-m gpu), against the oracle's analytic
k_grad rules (gradient, k_grad) and its finite-difference Hessian.

Bounds.  Gradient 1e-10 max|ref| (the bound of test_gpu_ops.py::test_predict_gradient_matches_contracted_k_grad): for
these seeds and trees the oracle's `dist + 1e-12` denominator and the exact one differ by <= 2.2e-12 relative, summation
order by ~2e-15.  Hessian 1e-6 max|ref| (test_gpu_estimators.py::test_predictor_hessian_and_log_determinant: the oracle
differentiates numerically).  k_grad 1e-12 max|ref|, 1e-9 with coincident rows (test_gpu_ops.py:538,557).  Route
equivalence 1e-10 max: both routes evaluate the same closed forms in fp64 and differ in the summation order over
m <= 257 terms -- m u sqrt(m) ~ 5e-13, times the O(10) cancellation of the monomial expansion."""
import numpy as np
import pytest

from oracle import mellon_oracle as mo

pytestmark = pytest.mark.gpu

D = 4
SHAPES = [(1, 1), (130, 70), (300, 257)]


def six_leaf(c):
    return (c.Matern52(1.5, active_dims=[0, 1]) * c.ExpQuad(2.5, active_dims=[2, 3])
            + c.Matern32(1.1, active_dims=[0, 2]) * c.Exponential(3.0, active_dims=[1, 3])
            + 0.5 * (c.RatQuad(2.0, 1.7, active_dims=[1, 2]) * c.ExpQuad(1.9, active_dims=[0, 3])))


def six_leaf_terms(c):
    return [c.Matern52(1.5, active_dims=[0, 1]) * c.ExpQuad(2.5, active_dims=[2, 3]),
            c.Matern32(1.1, active_dims=[0, 2]) * c.Exponential(3.0, active_dims=[1, 3]),
            0.5 * (c.RatQuad(2.0, 1.7, active_dims=[1, 2]) * c.ExpQuad(1.9, active_dims=[0, 3]))]


def deep_power(c):
    return ((c.Matern52(1.5, active_dims=[0, 1]) * c.ExpQuad(2.5, active_dims=[2, 3]) + 0.3)
            * (c.Matern32(1.1, active_dims=[0, 2]) + c.Exponential(3.0, active_dims=[1, 3]))
            * c.RatQuad(2.0, 1.7)) ** 1.5


def with_linear(c):
    return (c.Linear(2.0, active_dims=[0, 1]) * c.Matern52(1.5, active_dims=[1, 2])
            + c.ExpQuad(2.0, active_dims=[0, 3]) * c.Matern32(1.3) * c.RatQuad(1.5, 2.5, active_dims=[2, 3]))


TREES = {"six_leaf": six_leaf, "deep_power": deep_power}


@pytest.fixture(scope="module")
def ctx():
    from mellon_amd import _lib
    return _lib.default_context()


@pytest.fixture(autouse=True)
def small_row_blocks(monkeypatch):
    """n = 130 spans three row blocks, the last one ragged."""
    from mellon_amd.base_cov import BlockCov
    monkeypatch.setattr(BlockCov, "rows_per_block", 64)


_inputs_cache = {}


def inputs(n, m):
    if (n, m) not in _inputs_cache:
        seed = {(1, 1): 11, (130, 70): 12, (300, 257): 13}[(n, m)]
        rng = np.random.default_rng(seed)
        arrs = rng.normal(size=(n, D)), rng.normal(size=(m, D)), rng.normal(size=m)
        for a in arrs:
            a.setflags(write=False)
        _inputs_cache[(n, m)] = arrs
    return _inputs_cache[(n, m)]


_ref_cache = {}


def oracle_gradient(name, n, m):
    if (name, n, m) not in _ref_cache:
        xq, c, w = inputs(n, m)
        otree = {**TREES, "with_linear": with_linear}[name](mo)
        _ref_cache[(name, n, m)] = np.einsum("j,jik->ik", w, otree.k_grad(c)(xq))
    return _ref_cache[(name, n, m)]


def relmax(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def is_block(tree, d=D):
    from mellon_amd.base_cov import BlockCov
    return isinstance(tree.lower(d), BlockCov)


@pytest.mark.parametrize("n,m", SHAPES)
@pytest.mark.parametrize("name", sorted(TREES))
def test_gradient_matches_contracted_oracle_k_grad(ctx, name, n, m):
    from mellon_amd import cov
    tree = TREES[name](cov)
    assert is_block(tree)
    xq, c, w = inputs(n, m)
    g = ctx.predict_gradient(tree.lower(D), xq, c, w)
    ref = oracle_gradient(name, n, m)
    assert g.shape == (n, D)
    err = relmax(g, ref)
    print(f"gradient {name} ({n}, {m}): rel err {err:.3e}")
    assert err < 1e-10


@pytest.mark.parametrize("n,m", SHAPES)
def test_six_leaf_gradient_is_the_sum_of_its_one_program_terms(ctx, n, m):
    from mellon_amd import cov
    xq, c, w = inputs(n, m)
    g = ctx.predict_gradient(six_leaf(cov).lower(D), xq, c, w)
    parts = 0.0
    for term in six_leaf_terms(cov):
        assert not is_block(term)
        parts = parts + ctx.predict_gradient(term.lower(D), xq, c, w)
    err = relmax(g, parts)
    print(f"sum identity ({n}, {m}): rel err {err:.3e}")
    assert err < 1e-10


def _one_program_trees():
    from mellon_amd import cov
    a = cov.Matern52(1.3, active_dims=slice(None, -1))
    b = cov.Matern52(0.6, active_dims=-1)
    e = cov.ExpQuad(0.9, active_dims=[0, 2, 5])
    return [((a * b) + e * 0.5, 6),
            (cov.Matern52(1.5, active_dims=slice(None, -1)) * cov.Matern52(0.8, active_dims=-1), 4)]


@pytest.mark.parametrize("n,m", SHAPES)
@pytest.mark.parametrize("which", [0, 1])
def test_block_route_equals_the_one_program_route(ctx, which, n, m):
    """The same tree through both routes: BlockCov wrapped by hand against tree.lower(d)."""
    from mellon_amd.base_cov import BlockCov
    tree, d = _one_program_trees()[which]
    assert not is_block(tree, d)
    rng = np.random.default_rng(100 + n + m + which)
    xq, c, w = rng.normal(size=(n, d)), rng.normal(size=(m, d)), rng.normal(size=m)
    g1, g2 = ctx.predict_gradient(tree.lower(d), xq, c, w), ctx.predict_gradient(BlockCov(tree, d), xq, c, w)
    H1, H2 = ctx.predict_hessian(tree.lower(d), xq, c, w), ctx.predict_hessian(BlockCov(tree, d), xq, c, w)
    eg, eh = relmax(g2, g1), relmax(H2, H1)
    print(f"route equivalence tree {which} ({n}, {m}): gradient {eg:.3e} hessian {eh:.3e}")
    assert eg < 1e-10
    assert eh < 1e-10


@pytest.mark.parametrize("name", sorted(TREES))
def test_hessian_matches_oracle(ctx, name):
    from mellon_amd import cov
    from mellon_amd.base_predictor import Predictor
    n, m = 130, 70
    xq, c, w = inputs(n, m)
    tree, otree = TREES[name](cov), TREES[name](mo)
    H = ctx.predict_hessian(tree.lower(D), xq, c, w)
    ref = mo.Predictor(otree, c, w, 0.0, m).hessian(xq)
    assert H.shape == (n, D, D)
    sym = np.abs(H - np.swapaxes(H, 1, 2)).max() / np.abs(H).max()
    err = relmax(H, ref)
    print(f"hessian {name}: rel err {err:.3e} asymmetry {sym:.3e}")
    assert sym <= 1e-12
    assert err < 1e-6
    sign, _ = Predictor(tree, np.array(c), np.array(w), 0.0, n_obs=m).hessian_log_determinant(xq)
    assert np.array_equal(sign, np.linalg.slogdet(ref)[0])


def test_k_grad_of_a_six_leaf_tree(ctx):
    from mellon_amd import cov
    tree, otree = six_leaf(cov), six_leaf(mo)
    rng = np.random.default_rng(21)
    x, y = rng.normal(size=(40, D)), rng.normal(size=(33, D))
    g, ref = tree.k_grad(x)(y), otree.k_grad(x)(y)
    assert g.shape == (40, 33, D)
    err = relmax(g, ref)
    print(f"k_grad six_leaf: rel err {err:.3e}")
    assert err < 1e-12
    y2 = y.copy()
    y2[:5] = x[:5]                                    # coincident rows: distance floor 1e-6, delta = 0
    g2, r2 = tree.k_grad(x)(y2), otree.k_grad(x)(y2)
    err2 = np.abs(g2 - r2).max() / max(np.abs(r2).max(), 1.0)
    print(f"k_grad six_leaf, coincident rows: err {err2:.3e}")
    assert err2 < 1e-9


def test_linear_leaf_inside_a_five_leaf_tree(ctx):
    from mellon_amd import cov
    tree, otree = with_linear(cov), with_linear(mo)
    assert is_block(tree)
    n, m = 130, 70
    xq, c, w = inputs(n, m)
    g = ctx.predict_gradient(tree.lower(D), xq, c, w)
    eg = relmax(g, oracle_gradient("with_linear", n, m))
    H = ctx.predict_hessian(tree.lower(D), xq, c, w)
    ref = mo.Predictor(otree, c, w, 0.0, m).hessian(xq)
    eh = relmax(H, ref)
    print(f"linear leaf: gradient {eg:.3e} hessian {eh:.3e}")
    assert eg < 1e-10
    assert eh < 1e-6
    # the Linear-stationary cross terms live in H[0, 2] / H[2, 0] only through the first product: columns {0, 1} x {1, 2}
    assert np.abs(H - np.swapaxes(H, 1, 2)).max() <= 1e-12 * np.abs(H).max()
    kg, kref = tree.k_grad(xq[:40])(c[:33]), otree.k_grad(xq[:40])(c[:33])
    assert relmax(kg, kref) < 1e-12


def test_estimator_gradient_and_hessian(ctx):
    import mellon_amd
    from mellon_amd import cov
    from mellon_amd.base_predictor import ExpPredictor
    n, m = 1500, 60
    x = mo.gaussian_mixture(n, D, seed=17)
    nn = mo.exact_nn_distances(x)
    lm = mo.compute_landmarks(x, mo.SPARSE_CHOLESKY, m, 42)
    tree, otree = six_leaf(cov), six_leaf(mo)
    est = mellon_amd.DensityEstimator(cov_func=tree, landmarks=lm, nn_distances=nn)
    est.fit(x)
    q = x[::25] + 0.01
    op = mo.Predictor(otree, est.landmarks, est.predict.weights, est.mu, n)
    g, H = est.predict.gradient(q), est.predict.hessian(q)
    eg, eh = relmax(g, op.analytic_gradient(q)), relmax(H, op.hessian(q))
    print(f"estimator: gradient {eg:.3e} hessian {eh:.3e}")
    assert eg < 1e-10
    assert eh < 1e-6
    sign, _ = est.predict.hessian_log_determinant(q)
    assert np.array_equal(sign, np.linalg.slogdet(op.hessian(q))[0])
    # exp of a fitted function: grad e^f = e^f grad f, hess e^f = e^f (H_f + grad f grad f^T)
    y = np.sin(x[:, 0]) + 0.1 * x[:, 1]
    fest = mellon_amd.FunctionEstimator(cov_func=tree, sigma=0.1, landmarks=lm, nn_distances=nn).fit(x, y)
    fp = fest.predict
    ep = ExpPredictor.__new__(ExpPredictor)
    ep.__dict__.update(fp.__dict__)
    ofp = mo.Predictor(otree, fp.centers, fp.weights, fp.mu, n)
    f, gf, Hf = ofp(q), ofp.analytic_gradient(q), ofp.hessian(q)
    assert relmax(ep.gradient(q), np.exp(f)[:, None] * gf) < 1e-10
    assert relmax(ep.hessian(q), np.exp(f)[:, None, None] * (Hf + gf[:, :, None] * gf[:, None, :])) < 1e-6


def _user_matern52(with_k_grad):
    from mellon_amd.base_cov import Covariance

    class UserMatern52(Covariance):
        """The user's own Matern-5/2 of tests/test_gpu_round3.py, written in NumPy."""

        def __init__(self, ls=1.0, active_dims=None):
            super().__init__()
            self.ls = ls
            self.active_dims = active_dims

        def _sel(self, a):
            return a if self.active_dims is None else a[:, self.active_dims]

        def k(self, x, y):
            x, y = self._sel(x), self._sel(y)
            sq = (x * x).sum(1)[:, None] - 2.0 * x @ y.T + (y * y).sum(1)[None, :] + 1e-12
            r = np.sqrt(5.0) * np.sqrt(np.maximum(sq, 0.0)) / self.ls
            return (r + r * r / 3.0 + 1.0) * np.exp(-r)

    if with_k_grad:
        def k_grad(self, x):
            """The Matern-5/2 rule of the reference (cov.py:163-202): y -> d k(x, y) / d y, zero on inactive columns."""
            xs = self._sel(x)

            def grad(y):
                ys = self._sel(y)
                delta = ys[None, :, :] - xs[:, None, :]
                dist = np.sqrt(np.maximum((xs * xs).sum(1)[:, None] - 2.0 * xs @ ys.T + (ys * ys).sum(1)[None, :] + 1e-12, 0.0))
                f = np.sqrt(5.0) / self.ls
                r = f * dist
                coef = -(1.0 / 3.0) * np.exp(-r) * r * (r + 1.0) * f / (dist + 1e-12)
                out = np.zeros((x.shape[0], y.shape[0], x.shape[1]))
                cols = np.arange(x.shape[1]) if self.active_dims is None else np.arange(x.shape[1])[self.active_dims]
                out[:, :, cols] = coef[:, :, None] * delta
                return out

            return grad

        UserMatern52.k_grad = k_grad
    return UserMatern52


def test_user_leaf_with_its_own_k_grad(ctx):
    from mellon_amd import cov
    n, m = 130, 70
    xq, c, w = inputs(n, m)

    def build(first):
        return first * cov.ExpQuad(2.0, active_dims=[2, 3]) + 0.25 * cov.Matern32(0.9)

    User = _user_matern52(True)
    tree, plain = build(User(1.3, active_dims=[0, 1])), build(cov.Matern52(1.3, active_dims=[0, 1]))
    assert is_block(tree) and not is_block(plain)
    g, gp = ctx.predict_gradient(tree.lower(D), xq, c, w), ctx.predict_gradient(plain.lower(D), xq, c, w)
    eg = relmax(g, gp)
    kg, kp = tree.k_grad(xq[:40])(c[:33]), plain.k_grad(xq[:40])(c[:33])
    ek = relmax(kg, kp)
    print(f"user leaf: gradient {eg:.3e} k_grad {ek:.3e}")
    assert eg < 1e-10
    assert ek < 1e-12
    with pytest.raises(NotImplementedError, match="user-defined"):
        ctx.predict_hessian(tree.lower(D), xq, c, w)
    bare = build(_user_matern52(False)(1.3, active_dims=[0, 1]))
    with pytest.raises(NotImplementedError, match="k_grad"):
        ctx.predict_gradient(bare.lower(D), xq, c, w)
    with pytest.raises(NotImplementedError, match="k_grad"):
        bare.k_grad(xq[:5])(c[:5])
