"""The extended-precision restatement of the predictive mean (tests/predict_restatement.py) against the independently
written oracle, and the conditions the GPU tests (tests/test_gpu_predict_mean.py) put on their inputs.  No GPU."""
import numpy as np
import pytest

import predict_restatement as pr
from oracle import mellon_oracle as mo

# Per-value tolerances of a kernel entry (test_kernel_matrix_leaves, test_kernel_matrix_persistent_rows): TOLK off
# coincident pairs, TOLCO on them (distance < pr.CO_RADIUS), where the cancellation in xx - 2 xy + yy and not the
# sqrt / exp code sets the error.
# Reference against reference -- the largest |K_restated - oracle K| over all six kinds, d in {1, 33, 64}, n = 300,
# m = 130, on the recipe at its scaled counts and at (60, 60, 40) coincident / far / near rows:
#     off coincident pairs 3.6e-15  (Exponential, d = 1; on the far rows alone 6.8e-16 relative to the row's largest
#                                    entry (Linear), at most 4.4e-16 for RatQuad's polynomial tail: no figure of its own)
#     on coincident pairs  1.2e-8   (Exponential, d = 33, the cusp at 0; every other kind <= 1.2e-14)
# Both are below a quarter of their tolerance (2.5e-13, 2.5e-7), so the project's figures stand unchanged.
TOLK = 1e-12
TOLCO = 1e-6

DENSE = (60, 60, 40)      # more coincident and near pairs than the scaled recipe has at n = 300: a better sample of TOLCO


def _oracle(kind, params):
    return getattr(mo, kind)(*params)


def test_longdouble_is_wider_than_double():
    """The premise of the reference: at least the 64-bit significand of x87 extended precision."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


@pytest.mark.parametrize("kind", pr.KINDS)
@pytest.mark.parametrize("d", [1, 33, 64])
@pytest.mark.parametrize("counts", [None, DENSE], ids=["scaled", "dense"])
def test_restated_kernel_matrix_equals_oracle(kind, d, counts):
    n, m = 300, 130
    x, y, w = pr.make_inputs(n, m, d, 1000 * d + pr.KINDS.index(kind), counts)
    params = pr.kind_params(kind, d)
    mean, absdot, K, dist = pr.predict_mean_ref(kind, params, x, y, w, 0.25)
    ref = _oracle(kind, params)(x, y)
    tol, co = pr.pair_tolerance(K, dist, TOLK, TOLCO)
    err = np.abs(K - ref)
    print(f"{kind} d={d}: off {(err / tol * TOLK)[~co].max():.3e} on {(err / tol * TOLCO)[co].max():.3e}")
    assert np.all(err <= tol)
    # a quarter of the tolerance: the margin that lets the tolerances stand as the project has them (see above)
    assert np.all(err <= tol / 4)
    h, far, near = counts or pr.recipe_counts(n)
    assert np.allclose(np.asarray(dist, dtype=np.float64)[np.arange(h), np.arange(h)], 1e-6, rtol=1e-15, atol=0)
    assert co[h + far:h + far + near, m - near:].diagonal().all()
    assert co.sum() >= h + near
    if d > 1:                                              # (one column: a cell times 400 can still lie among the centres)
        assert not co[h:h + far].any()                     # the far rows: far from everything
        if kind != "Linear":
            assert K[h:h + far].max() < (1e-8 if kind == "RatQuad" else 1e-100)     # e^-r is gone,
            assert K[h:h + far].min() > (0.0 if kind == "RatQuad" else -1.0)        # RatQuad's tail has not
    assert ((np.abs(K) > 1e-3) & ~co).sum() >= min(10000, n * m // 4)
    # the mean and absdot are the longdouble sums of that matrix
    assert np.abs(np.asarray(mean, dtype=np.float64) - (0.25 + ref @ w)).max() <= pr.row_bound(K, dist, w, absdot, TOLK, TOLCO).max()
    assert np.allclose(np.asarray(absdot, dtype=np.float64), np.abs(ref * w).sum(axis=1), rtol=1e-9)


def test_restated_active_dims_and_algebra_equal_oracle():
    """Leaves over column subsets (index list, boolean mask, slice, scalar) and the product / sum built from them."""
    x, y, w = pr.make_inputs(130, 67, 6, 5)
    mask = np.array([True, False, True, False, False, True])
    for kind, ad in (("ExpQuad", [0, 2, 5]), ("Matern32", mask), ("Matern52", slice(None, -1)), ("Exponential", -1)):
        K, dist = pr.kernel_ref(kind, (1.3,), x, y, ad)
        tol, _ = pr.pair_tolerance(K, dist, TOLK, TOLCO)
        assert np.all(np.abs(K.astype(np.float64) - getattr(mo, kind)(1.3, active_dims=ad)(x, y)) <= tol / 4)
    K0, d0 = pr.kernel_ref("Matern52", (1.3,), x, y, slice(None, -1))
    K1, d1 = pr.kernel_ref("Exponential", (0.6,), x, y, -1)
    a, b = mo.Matern52(1.3, active_dims=slice(None, -1)), mo.Exponential(0.6, active_dims=-1)
    for K, ref in ((K0 * K1, (a * b)(x, y)), (K0 + K1, (a + b)(x, y))):
        tol, _ = pr.pair_tolerance(K, np.minimum(d0, d1), TOLK, TOLCO)      # coincident in either leaf
        assert np.all(np.abs(K.astype(np.float64) - ref) <= tol / 4)
    mean, absdot = pr.mean_of(K0 * K1, w, 0.0)
    assert np.abs(np.asarray(mean, dtype=np.float64) - (a * b)(x, y) @ w).max() < 1e-13 * float(absdot.max())


@pytest.mark.parametrize("n,m,d", [(4096, 256, 1), (4096, 256, 8), (4100, 383, 33), (4223, 448, 64), (300, 130, 130),
                                   (130, 67, 6), (64, 64, 3), (63, 65, 3)])
def test_input_conditions_at_the_gpu_shapes(n, m, d):
    """What the GPU tests assert about their inputs, checked here at their shapes: few rows carry the loose coincident
    tolerance, and enough entries are neither negligible nor coincident for the tight one to bite."""
    x, y, w = pr.make_inputs(n, m, d, 7 * d + n)
    K, dist = pr.kernel_ref("Matern52", pr.kind_params("Matern52", d), x, y)
    co = np.asarray(dist < pr.CO_RADIUS)
    h, far, near = pr.recipe_counts(n)
    assert co.sum() >= h + near
    if d == 1:
        # one column: every cell has centres within 0.05 by chance, so the share is taken over pairs instead of rows
        assert co.mean() <= 0.05
    else:
        assert co.any(axis=1).mean() <= 0.05
    assert ((K > 1e-3) & ~co).sum() >= min(10000, n * m // 4)
    assert far >= 1 and (d == 1 or K[h:h + far].max() < 1e-100)       # rows on which e^-r is gone
