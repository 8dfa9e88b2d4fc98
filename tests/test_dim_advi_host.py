"""optimizer="advi" of the DimensionalityEstimator on the host: the entry point is declared and bound, the NumPy
restatement the device tests compare against (tests/dim_advi_restatement.py) has the gradients of its own value, and
inference.run_advi walks the restatement's loop bit for bit on (2, m) parameters."""
import os
import re

import numpy as np

import dim_advi_restatement as dar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batched_dimensionality_objective_is_declared_and_bound():
    from mellon_amd import _lib
    header = open(os.path.join(ROOT, "include", "mellon_hip.h")).read()
    assert re.search(r"^int\s+mln_dim_objective_batch\s*\(", header, flags=re.M)
    bound = {s[0]: s for s in _lib.SYMBOLS}
    assert "mln_dim_objective_batch" in bound
    assert len(bound["mln_dim_objective_batch"][2]) == 5          # fit, Z, S, loss, grad
    assert hasattr(_lib.Fit, "dim_objective_batch")
    from mellon_amd import _build
    assert "dim_objective_batch.hip" in _build.SOURCES


def test_restatement_gradients_against_finite_differences():
    n, m, k, S = 60, 8, 5, 3
    L, ell, mu_dim, mu_dens = dar.synthetic(n, m, k, seed=11)
    rng = np.random.default_rng(3)
    mean = 0.2 * rng.standard_normal((2, m))
    log_std = -1.0 + 0.3 * rng.standard_normal((2, m))
    eps = dar.advi_draws(5, S, 2 * m)
    args = (L, ell, mu_dim, mu_dens)
    value, gm, gs = dar.elbo_value_and_grad(mean, log_std, eps, *args)
    assert np.isfinite(value) and gm.shape == (2, m) and gs.shape == (2, m)
    h = 1e-5
    for i in range(2):
        for j in range(m):
            e = np.zeros((2, m))
            e[i, j] = h
            fm = (dar.elbo_value_and_grad(mean + e, log_std, eps, *args)[0]
                  - dar.elbo_value_and_grad(mean - e, log_std, eps, *args)[0]) / (2 * h)
            fs = (dar.elbo_value_and_grad(mean, log_std + e, eps, *args)[0]
                  - dar.elbo_value_and_grad(mean, log_std - e, eps, *args)[0]) / (2 * h)
            # central differences: truncation h^2 f''' / 6 ~ 1e-10 relative, rounding eps |value| / h ~ 1e-8 absolute
            assert abs(fm - gm[i, j]) < 1e-6 * max(1.0, np.abs(gm).max()), (i, j, fm, gm[i, j])
            assert abs(fs - gs[i, j]) < 1e-6 * max(1.0, np.abs(gs).max()), (i, j, fs, gs[i, j])
    # the flat form is the same computation
    v2, gm2, gs2 = dar.elbo_value_and_grad(mean.ravel(), log_std.ravel(), eps, *args)
    assert v2 == value and np.array_equal(gm2, gm.ravel()) and np.array_equal(gs2, gs.ravel())


class NumpyDimLoss:
    """What run_advi needs of a loss: value_and_grad_batch over the flat (S, 2 m) points, here the restatement's."""

    def __init__(self, *args):
        self.args = args
        self.n_eval = 0
        self.shapes = []

    def value_and_grad_batch(self, Z):
        self.n_eval += Z.shape[0]
        self.shapes.append(Z.shape)
        return dar.losses_and_grads(Z, *self.args)


def test_run_advi_reproduces_the_restatement_loop_on_two_row_parameters():
    from mellon_amd import inference
    n, m, k = 60, 8, 5
    L, ell, mu_dim, mu_dens = dar.synthetic(n, m, k, seed=12)
    z0 = 0.1 * np.random.default_rng(1).standard_normal((2, m))
    want = dar.run_advi(z0, L, ell, mu_dim, mu_dens, n_iter=6, nsamples=5)
    loss = NumpyDimLoss(L, ell, mu_dim, mu_dens)
    got = inference.run_advi(loss, z0, n_iter=6, nsamples=5)
    assert loss.n_eval == 6 * 5 and set(loss.shapes) == {(5, 2 * m)}
    assert got.pre_transformation.shape == (2, m) and got.pre_transformation_std.shape == (2, m)
    assert np.array_equal(got.pre_transformation, want[0])
    assert np.array_equal(got.pre_transformation_std, want[1]) and np.all(want[1] > 0)
    assert np.array_equal(np.asarray(got.losses), want[2]) and np.isfinite(want[2]).all()
    # what DimensionalityEstimator.run_inference does with them
    assert np.asarray(got.pre_transformation_std).reshape(2, -1).shape == (2, m)
