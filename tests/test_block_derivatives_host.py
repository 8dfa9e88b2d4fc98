"""The tree walk of mellon_amd/block_derivatives.py on the NumPy backend (no GPU): the first / second derivatives of a
covariance tree with respect to its leaf values against central differences, and the column lists every leaf ends up with."""
import numpy as np
import pytest

from mellon_amd import block_derivatives as bd
from mellon_amd import cov
from mellon_amd.base_cov import Mul


def six_leaf(c):
    """The tree of tests/test_gpu_round3.py::test_six_leaf_sum_of_products."""
    return (c.Matern52(1.5, active_dims=[0, 1]) * c.ExpQuad(2.5, active_dims=[2, 3])
            + c.Matern32(1.1, active_dims=[0, 2]) * c.Exponential(3.0, active_dims=[1, 3])
            + 0.5 * (c.RatQuad(2.0, 1.7, active_dims=[1, 2]) * c.ExpQuad(1.9, active_dims=[0, 3])))


def deep_power(c):
    return ((c.Matern52(1.5, active_dims=[0, 1]) * c.ExpQuad(2.5, active_dims=[2, 3]) + 0.3)
            * (c.Matern32(1.1, active_dims=[0, 2]) + c.Exponential(3.0, active_dims=[1, 3]))
            * c.RatQuad(2.0, 1.7)) ** 1.5


TREES = {"six_leaf": six_leaf, "deep_power": deep_power}


@pytest.mark.parametrize("name", sorted(TREES))
def test_leaf_derivatives_match_central_differences(name):
    """a_l = dP/dk_l and b_ll' = d2P/dk_l dk_l' of the walk against central differences of P in the leaf values.
    Leaf values in [0.5, 1.5] keep P and its derivatives O(1 .. 10).  Step 1e-5 for the first derivative: truncation
    ~ step^2 P''' ~ 1e-9, rounding ~ 1e-16 / step = 1e-11 -> bound 1e-7 of the largest entry.  Step 1e-3 for the second
    differences: truncation ~ step^2 P'''' ~ 1e-5, rounding ~ 4e-16 / step^2 = 4e-10 -> bound 1e-4."""
    tree = TREES[name](cov)
    leaves, plan = bd.collect_leaves(tree, 4)
    L = len(leaves)
    assert L == (6 if name == "six_leaf" else 5)
    rng = np.random.default_rng(7)
    vals = [rng.uniform(0.5, 1.5, size=(5, 7)) for _ in range(L)]
    be = bd.NumpyBlocks()

    def P(shift):
        return bd.propagate(plan, [v + shift.get(i, 0.0) for i, v in enumerate(vals)], be)[0]

    value, a1, a2 = bd.propagate(plan, vals, be, second=True)
    _, a1_only, none = bd.propagate(plan, vals, be)
    assert none == {} and sorted(a1_only) == sorted(a1) == list(range(L))
    scale1 = max(np.abs(np.broadcast_to(a1[l], value.shape)).max() for l in range(L))
    h1, h2 = 1e-5, 1e-3
    for l in range(L):
        fd = (P({l: h1}) - P({l: -h1})) / (2 * h1)
        assert np.abs(np.broadcast_to(a1[l], fd.shape) - fd).max() < 1e-7 * scale1, l
        assert np.array_equal(np.broadcast_to(a1[l], fd.shape), np.broadcast_to(a1_only[l], fd.shape))
    fds = {}
    for l in range(L):
        for lp in range(l, L):
            if l == lp:
                fds[(l, lp)] = (P({l: h2}) - 2.0 * P({}) + P({l: -h2})) / (h2 * h2)
            else:
                fds[(l, lp)] = (P({l: h2, lp: h2}) - P({l: h2, lp: -h2}) - P({l: -h2, lp: h2})
                                + P({l: -h2, lp: -h2})) / (4 * h2 * h2)
    scale2 = max(np.abs(v).max() for v in fds.values())
    assert scale2 > 0.1
    for key, fd in fds.items():
        got = np.broadcast_to(a2[key], fd.shape) if key in a2 else np.zeros_like(fd)     # absent: identically zero
        assert np.abs(got - fd).max() < 1e-4 * scale2, key
    assert all(l <= lp for l, lp in a2)
    if name == "six_leaf":      # a sum of two-leaf products: only the three in-term mixed partials exist
        assert sorted(a2) == [(0, 1), (2, 3), (4, 5)]
        assert isinstance(a1[0], np.ndarray) and np.array_equal(a1[0], vals[1])
        assert np.array_equal(a2[(4, 5)], 0.5) or a2[(4, 5)] == 0.5


def test_same_leaf_object_twice_counts_as_two_leaves():
    a = cov.Matern52(1.3)
    leaves, plan = bd.collect_leaves(a * a + a, 3)
    assert len(leaves) == 3 and all(lf.node is a for lf in leaves)
    rng = np.random.default_rng(0)
    v = rng.uniform(0.5, 1.5, size=(3, 4))
    value, a1, a2 = bd.propagate(plan, [v, v, v], bd.NumpyBlocks(), second=True)
    assert np.allclose(value, v * v + v)
    assert np.array_equal(a1[0], v) and np.array_equal(a1[1], v) and a1[2] == 1.0
    assert list(a2) == [(0, 1)] and a2[(0, 1)] == 1.0


@pytest.mark.parametrize("d", [4, 6])
def test_composite_active_dims_reach_the_leaves_as_emit_gives_them(d):
    trees = [six_leaf(cov), deep_power(cov),
             Mul(cov.ExpQuad(0.9, active_dims=[1, 2]), cov.Matern32(1.1, active_dims=slice(None, -1)), active_dims=[3, 0, 2])
             + cov.Matern52(1.0, active_dims=-1) * cov.Linear(2.0, active_dims=np.arange(d) % 2 == 0)]
    for tree in trees:
        emitted, toks = [], []
        tree._emit(np.arange(d), emitted, toks)
        leaves, _ = bd.collect_leaves(tree, d)
        assert len(leaves) == len(emitted)
        for lf, (kind, ls, alpha, dims) in zip(leaves, emitted):
            assert not lf.user and lf.kind == kind and lf.ls == ls and lf.alpha == alpha
            assert lf.dims.dtype == np.int32 and list(lf.dims) == list(dims)
    nested = bd.collect_leaves(trees[2], d)[0]
    assert list(nested[0].dims) == [0, 2] and list(nested[1].dims) == [3, 0]      # composite columns first, then the leaf's


def test_rows_per_block_keeps_the_live_blocks_within_the_budget():
    for ld, n_live in ((16, 30), (5008, 30), (5008, 70), (100_000, 70)):
        rows = bd._rows_per_block(8192, ld, n_live)
        assert 64 <= rows <= 8192
        assert rows == 64 or rows * ld * n_live * 8 <= bd.BLOCK_BYTES


def test_user_leaf_without_k_grad_is_refused_before_any_device_work():
    from mellon_amd.base_cov import BlockCov, Covariance

    class Mine(Covariance):
        def k(self, x, y):
            return x @ y.T

    bc = (Mine() * cov.ExpQuad(1.0)).lower(3)
    assert isinstance(bc, BlockCov)
    x = np.zeros((2, 3))
    with pytest.raises(NotImplementedError, match="k_grad"):
        bd.predict_gradient(None, bc, x, x, np.ones(2))
    with pytest.raises(NotImplementedError, match="k_grad"):
        bd.kernel_grad(None, bc, x, x)
    with pytest.raises(NotImplementedError, match="user-defined"):
        bd.predict_hessian(None, bc, x, x, np.ones(2))


# ---- the whole contraction in NumPy: the walk + hessian_coefficients + the sums the device entries evaluate ----------
def with_linear(c):
    return (c.Linear(2.0, active_dims=[0, 1]) * c.Matern52(1.5, active_dims=[1, 2])
            + c.ExpQuad(2.0, active_dims=[0, 3]) * c.Matern32(1.3) * c.RatQuad(1.5, 2.5, active_dims=[2, 3]))


def _leaf_factors(lf, x, c):
    """K, g, h of one built-in leaf as csrc/cov_leaf.h defines them (exact denominator)."""
    from mellon_amd import _lib
    xs, cs = x[:, lf.dims], c[:, lf.dims]
    xy, il = xs @ cs.T, 1.0 / lf.ls
    if lf.linear:
        return xy * il, np.full_like(xy, il), np.zeros_like(xy)
    sq = (xs * xs).sum(1)[:, None] - 2 * xy + (cs * cs).sum(1)[None, :] + 1e-12
    dist = np.sqrt(sq)
    if lf.kind == _lib.K_MATERN32:
        f = np.sqrt(3) * il
        r, e = f * dist, np.exp(-f * dist)
        return (r + 1) * e, -f * r * e / dist, f ** 3 * e / dist
    if lf.kind == _lib.K_MATERN52:
        f = np.sqrt(5) * il
        r, e = f * dist, np.exp(-f * dist)
        return (r + r * r / 3 + 1) * e, -e * r * (r + 1) * f / dist / 3, f ** 4 * e / 3
    if lf.kind == _lib.K_EXPQUAD:
        r = dist * il
        e = np.exp(-0.5 * r * r)
        return e, -r * il * e / dist, e * il ** 4
    if lf.kind == _lib.K_EXPONENTIAL:
        e = np.exp(-0.5 * dist * il)
        return e, -0.5 * il * e / dist, e * (0.25 * il * il / sq + 0.5 * il / (sq * dist))
    r = dist * il
    b = r * r / (2 * lf.alpha) + 1
    return b ** -lf.alpha, -r * il * b ** (-lf.alpha - 1) / dist, (lf.alpha + 1) / lf.alpha * b ** (-lf.alpha - 2) * il ** 4


@pytest.mark.parametrize("build", [six_leaf, deep_power, with_linear], ids=["six_leaf", "deep_power", "with_linear"])
def test_numpy_contraction_matches_the_oracle(build):
    """Gradient within 1e-10 of the oracle's contracted k_grad (its dist + 1e-12 denominator costs ~2e-12), Hessian within
    1e-6 of its finite-difference Hessian: the bounds of the device tests, on the formulas the device entries implement."""
    from oracle import mellon_oracle as mo
    n, m, d = 40, 23, 4
    rng = np.random.default_rng(12)
    xq, c, w = rng.normal(size=(n, d)), rng.normal(size=(m, d)), rng.normal(size=m)
    tree, otree = build(cov), build(mo)
    be = bd.NumpyBlocks()
    leaves, plan = bd.collect_leaves(tree, d)
    L = len(leaves)
    F = [_leaf_factors(lf, xq, c) for lf in leaves]
    vals, g, h = [f[0] for f in F], {i: f[1] for i, f in enumerate(F)}, {i: f[2] for i, f in enumerate(F)}
    value, a1, a2 = bd.propagate(plan, vals, be, second=True)
    assert np.abs(value - otree(xq, c)).max() < 1e-13 * np.abs(value).max()
    grad = np.zeros((n, d))
    for i, lf in enumerate(leaves):
        Q = bd._mul(be, a1[i], g[i]) * w[None, :]
        if lf.linear:
            grad[:, lf.dims] += Q @ c[:, lf.dims]
        else:
            grad[:, lf.dims] += xq[:, lf.dims] * Q.sum(1)[:, None] - Q @ c[:, lf.dims]
    ref = np.einsum("j,jik->ik", w, otree.k_grad(c)(xq))
    assert np.abs(grad - ref).max() < 1e-10 * np.abs(ref).max()
    Qd, Qp = bd.hessian_coefficients(be, leaves, vals, g, h, a1, a2)
    assert len(Qd) == L and len(Qp) == L * (L + 1) // 2
    H, slot, rows = np.zeros((n, d, d)), 0, np.arange(n)
    for l in range(L):
        if Qd[l] is not None:
            for dim in leaves[l].dims:
                H[:, dim, dim] += (Qd[l] * w).sum(1)
        for lp in range(l, L):
            q, slot = Qp[slot], slot + 1
            if q is None:
                continue
            sa, sb = (0.0 if leaves[l].linear else 1.0), (0.0 if leaves[lp].linear else 1.0)
            da = sa * xq[:, None, leaves[l].dims] - c[None, :, leaves[l].dims]
            db = sb * xq[:, None, leaves[lp].dims] - c[None, :, leaves[lp].dims]
            M = np.einsum("ij,ija,ijb->iab", q * w, da, db)
            H[np.ix_(rows, leaves[l].dims, leaves[lp].dims)] += M
            if lp != l:
                H[np.ix_(rows, leaves[lp].dims, leaves[l].dims)] += M.transpose(0, 2, 1)
    Href = mo.Predictor(otree, c, w, 0.0, m).hessian(xq)
    assert np.abs(H - Href).max() < 1e-6 * np.abs(Href).max()
