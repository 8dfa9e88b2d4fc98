"""optimizer="advi" on a real MI355X (-m gpu): the batched objective (mln_objective_batch) against single passes and the
oracle, sharded against unsharded, run_advi against the NumPy restatement (tests/advi_restatement.py) with the same
draws, and the estimator surface of the reference's tests/test_density_estimator.py:165-234 with the real optimiser.

Tolerances: the batched objective is held to what the suite holds mln_objective to (tests/test_gpu_ops.py: loss 1e-11
relative, gradient 1e-8 of its largest entry).  run_advi against the restatement: 1e-6 -- relative noise of 1e-9 in every
gradient of the restatement moves the 100-step result by at most 2.7e-10 (mean), 6.4e-10 (std), 3.6e-10 (losses) on the
three shapes below (Adam does not amplify it), so gradient parity at 1e-8 leaves about two orders of margin."""
import json

import numpy as np
import pytest

import advi_restatement as ar
from oracle import mellon_oracle as mo

pytestmark = pytest.mark.gpu

S_VALUES = [1, 2, 15, 16, 17, 40, 64, 65, 130]


@pytest.fixture(scope="module")
def mellon():
    import mellon_amd
    return mellon_amd


@pytest.fixture(scope="module")
def ctx():
    from mellon_amd import _lib
    return _lib.default_context()


def relmax(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _check_batch(fit, Z, L=None, mu=None, V=None, Vdr=None, tag=""):
    """objective_batch(Z) against len(Z) single passes on the same handle and (given L) the oracle; identical bits twice."""
    loss, grad = fit.objective_batch(Z)
    assert loss.shape == (len(Z),) and grad.shape == Z.shape
    loss2, grad2 = fit.objective_batch(Z)
    assert np.array_equal(loss, loss2) and np.array_equal(grad, grad2)
    singles = [fit.objective(z) for z in Z]
    l1 = np.array([s[0] for s in singles])
    g1 = np.stack([s[1] for s in singles])
    e_loss = np.abs(loss - l1) / np.abs(l1)
    e_grad = max(relmax(grad[s], g1[s]) for s in range(len(Z)))
    print(f"{tag} S={len(Z)} m={Z.shape[1]}: vs single passes loss {e_loss.max():.2e} grad {e_grad:.2e}", end="")
    assert e_loss.max() < 1e-11 and e_grad < 1e-8
    if L is not None:
        ref = [mo.loss_and_grad(z, L, mu, V, Vdr) for z in Z]
        o_loss = max(abs(loss[s] - ref[s][0]) / abs(ref[s][0]) for s in range(len(Z)))
        o_grad = max(relmax(grad[s], ref[s][1]) for s in range(len(Z)))
        print(f"; vs oracle loss {o_loss:.2e} grad {o_grad:.2e}", end="")
        assert o_loss < 1e-11 and o_grad < 1e-8
    print()


def _problem(n, d, m, seed):
    x = mo.gaussian_mixture(n, d, seed)
    nn = mo.exact_nn_distances(x)
    ls, mu = mo.compute_ls(nn), mo.compute_mu(nn, d)
    rng = np.random.default_rng(seed)
    xu = x[rng.choice(n, size=m, replace=False)] + 0.01 * rng.normal(size=(m, d))
    return x, nn, ls, mu, xu


# ---- 1. the batched objective -------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,S", [(1, 300, 17), (3, 1501, 2), (16, 1501, 16), (17, 1501, 65), (100, 3001, 40),
                                   (1000, 1501, 15), (5000, 1501, 40), (5000, 777, 1)])
def test_batch_landmark_counts(ctx, m, n, S):
    """Every accumulator width and row / column tail of the two kernels on a given factor (Fit.from_L)."""
    from mellon_amd import _lib
    rng = np.random.default_rng(1000 * m + S)
    L = rng.normal(size=(n, m)) * (0.5 / np.sqrt(m))
    V, Vdr = mo.nn_likelihood_constants(rng.uniform(0.2, 1.0, size=n), 5)
    fit = _lib.Fit.from_L(ctx, L)
    fit.set_likelihood(V, Vdr, -3.0)
    Z = rng.normal(size=(S, m)) * 0.3
    _check_batch(fit, Z, L, -3.0, V, Vdr, tag="from_L")
    fit.close()


@pytest.mark.parametrize("S", S_VALUES)
def test_batch_sample_counts(ctx, S):
    """Every chunking of S (one to three launches, every padding of the last one) on one factor."""
    from mellon_amd import _lib
    n, m = 2049, 100
    rng = np.random.default_rng(S)
    L = rng.normal(size=(n, m)) * (0.5 / np.sqrt(m))
    V, Vdr = mo.nn_likelihood_constants(rng.uniform(0.2, 1.0, size=n), 5)
    fit = _lib.Fit.from_L(ctx, L)
    fit.set_likelihood(V, Vdr, -3.0)
    _check_batch(fit, rng.normal(size=(S, m)) * 0.3, L, -3.0, V, Vdr, tag="from_L")
    fit.close()


@pytest.mark.parametrize("kind", ["explicit", "implicit", "full", "sparse_nystroem", "full_nystroem"])
def test_batch_handle_kinds(ctx, kind):
    """The handle layouts of the four gp types: explicit and implicit sparse Cholesky, the full GP, both Nystroem kinds."""
    from mellon_amd import cov
    n, d, m = (700, 5, 0) if kind in ("full", "full_nystroem") else (3001, 3, 130)
    x, nn, ls, mu, xu = _problem(n, d, max(m, 1), seed=n + m)
    c = cov.Matern52(ls)
    V, Vdr = mo.nn_likelihood_constants(nn, d)
    base = ctx.fit_prepare(c.lower(d), x, None if m == 0 else xu, 1e-6, implicit=(kind == "implicit"))
    fit = base
    if kind.endswith("nystroem"):
        base.gram_eigh()
        fit = base.project(57)
    fit.set_likelihood(V, Vdr, mu)
    L = fit.L()
    rng = np.random.default_rng(5)
    z0 = mo.compute_initial_value(nn, d, mu, L)
    for S in (40, 17):
        Z = z0[None, :] + 0.05 * rng.normal(size=(S, fit.m))
        _check_batch(fit, Z, L, mu, V, Vdr, tag=kind)


def test_batch_per_cell_dimensionality(ctx):
    """`d` given per cell: V and Vdr are vectors with a different constant in every row."""
    from mellon_amd import cov
    n, d, m = 2500, 4, 64
    x, nn, ls, mu, xu = _problem(n, d, m, seed=21)
    dd = np.random.default_rng(2).uniform(2.0, 6.0, size=n)
    V, Vdr = mo.nn_likelihood_constants(nn, dd)
    fit = ctx.fit_prepare(cov.Matern52(ls).lower(d), x, xu, 1e-6)
    fit.set_likelihood(V, Vdr, mu)
    L = fit.L()
    Z = 0.1 * np.random.default_rng(3).normal(size=(40, m))
    _check_batch(fit, Z, L, mu, V, Vdr, tag="per-cell d")


def test_batch_argument_errors(ctx):
    from mellon_amd import _lib
    L = np.random.default_rng(0).normal(size=(50, 7))
    fit = _lib.Fit.from_L(ctx, L)
    with pytest.raises(Exception):
        fit.objective_batch(np.zeros((3, 7)))          # no likelihood yet
    fit.set_likelihood(np.zeros(50), np.zeros(50), 0.0)
    with pytest.raises(ValueError):
        fit.objective_batch(np.zeros((3, 8)))
    with pytest.raises(ValueError):
        fit.objective_batch(np.zeros((0, 7)))
    fit.close()


# ---- 2. sharded ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ranks", [2, 3])
@pytest.mark.parametrize("implicit", [False, True])
def test_batch_sharded(ctx, n_ranks, implicit):
    """Uneven shards on loopback thread-ranks: one all-reduce of the losses and the gradient block, prior terms once."""
    from mellon_amd import cov, distributed
    n, d, m = 3001, 3, 130
    x, nn, ls, mu, xu = _problem(n, d, m, seed=77)
    desc = cov.Matern52(ls).lower(d)
    V, Vdr = mo.nn_likelihood_constants(nn, d)
    Z = 0.1 * np.random.default_rng(8).normal(size=(40, m))
    one = ctx.fit_prepare(desc, x, xu, 1e-6, implicit=implicit)
    one.set_likelihood(V, Vdr, mu)
    loss1, grad1 = one.objective_batch(Z)
    cuts = [0] + [int(n * f) for f in ((0.37,) if n_ranks == 2 else (0.2, 0.71))] + [n]

    def body(comm):
        lo, hi = cuts[comm.rank], cuts[comm.rank + 1]
        f = comm.ctx.fit_prepare(desc, np.ascontiguousarray(x[lo:hi]), xu, 1e-6, implicit=implicit)
        f.set_likelihood(V[lo:hi], Vdr[lo:hi], mu)
        out = f.objective_batch(Z)
        f.close()
        return out

    res = distributed.run_loopback(n_ranks, body)
    for loss, grad in res:
        assert np.array_equal(loss, res[0][0]) and np.array_equal(grad, res[0][1])     # same bits on every rank
        e_loss, e_grad = (np.abs(loss - loss1) / np.abs(loss1)).max(), relmax(grad, grad1)
        print(f"{n_ranks} ranks implicit={implicit}: loss {e_loss:.2e} grad {e_grad:.2e}")
        assert e_loss < 1e-11 and e_grad < 1e-8


# ---- 3. run_advi against the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,n_landmarks", [(200, 2, 20), (2000, 5, 100), (5000, 10, 300)])
def test_run_advi_against_restatement(mellon, ctx, n, d, n_landmarks):
    from mellon_amd import inference
    X = ar.two_blobs(n, d)
    ref = mo.density_fit(X, n_landmarks=n_landmarks)
    V, Vdr = mo.nn_likelihood_constants(ref.nn_distances, ref.d)
    want = ar.run_advi(ref.initial_value, ref.L, ref.mu, V, Vdr, n_iter=100)
    transform = inference.compute_transform(ref.mu, ref.L)
    loss_func = inference.compute_loss_func(ref.nn_distances, ref.d, transform, ref.L.shape[1])
    got = inference.run_advi(loss_func, ref.initial_value, n_iter=100)
    assert loss_func.n_eval == 100 * 40
    e_mean = np.abs(got.pre_transformation - want[0]).max()
    e_std = np.abs(got.pre_transformation_std / want[1] - 1).max()
    e_loss = np.abs(np.asarray(got.losses) / want[2] - 1).max()
    print(f"n={n} d={d} m={ref.L.shape[1]}: |dmean| {e_mean:.2e} rel dstd {e_std:.2e} rel dlosses {e_loss:.2e}")
    assert len(got.losses) == 100
    assert e_mean < 1e-6 and e_std < 1e-6 and e_loss < 1e-6


# ---- 4. the estimators ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_x():
    return ar.two_blobs(100, 2, seed=1)


@pytest.mark.parametrize("rank,n_landmarks", [(1.0, 0), (0.99, 0), (1.0, 10), (0.99, 80)])
def test_density_estimator_advi_uncertainty(mellon, small_x, tmp_path, rank, n_landmarks):
    n = small_x.shape[0]
    est = mellon.DensityEstimator(rank=rank, n_landmarks=n_landmarks, optimizer="advi", predictor_with_uncertainty=True,
                                  n_iter=30)
    dens = est.fit_predict(small_x)
    assert dens.shape == (n,) and np.isfinite(dens).all()
    assert est.pre_transformation_std is not None and est.pre_transformation_std.shape == est.pre_transformation.shape
    assert np.all(est.pre_transformation_std > 0)
    assert len(est.losses) == 30 and np.isfinite(est.losses).all()
    assert est.opt_state is None                                     # ADVI leaves it untouched (base_model.py:390-400)
    p = est.predict
    assert p.covariance(small_x).shape == (n,) and p.covariance(small_x, diag=False).shape == (n, n)
    assert p.mean_covariance(small_x).shape == (n,) and p.mean_covariance(small_x, diag=False).shape == (n, n)
    unc = p.uncertainty(small_x)
    assert unc.shape == (n,) and p.uncertainty(small_x, diag=False).shape == (n, n)
    path = str(tmp_path / f"advi_{n_landmarks}_{rank}.json")
    p.to_json(path)
    again = mellon.Predictor.from_json(path)
    assert np.allclose(again(small_x), p(small_x)) and np.allclose(again.uncertainty(small_x), unc)
    json.loads(p.to_json())


def test_density_estimator_advi_without_uncertainty(mellon, small_x):
    est = mellon.DensityEstimator(optimizer="advi", n_iter=25)
    est.fit(small_x)
    assert est.pre_transformation_std is not None and est.pre_transformation_std.shape == est.pre_transformation.shape
    assert len(est.losses) == 25
    # a second fit reproduces the first: the draws are keyed by the step
    est2 = mellon.DensityEstimator(optimizer="advi", n_iter=25)
    est2.fit(small_x)
    assert np.array_equal(est2.pre_transformation, est.pre_transformation) and est2.losses == est.losses


def test_advi_density_correlates_with_map(mellon):
    """The reference's own property (tests/test_laplace.py:170-193 there) on the device."""
    X = ar.two_blobs(200, 2)
    dens_map = mellon.DensityEstimator(n_landmarks=20).fit_predict(X)
    est = mellon.DensityEstimator(n_landmarks=20, optimizer="advi", n_iter=200)
    dens_advi = est.fit_predict(X)
    corr = np.corrcoef(dens_map, dens_advi)[0, 1]
    print(f"corr(MAP, ADVI) = {corr:.4f}")
    assert corr > 0.8


def test_time_sensitive_estimator_advi(mellon):
    rng = np.random.default_rng(4)
    x = np.concatenate([rng.standard_normal((60, 2)) * 0.5 + t for t in range(3)])
    times = np.repeat(np.arange(3.0), 60)
    est = mellon.TimeSensitiveDensityEstimator(optimizer="advi", n_iter=20, n_landmarks=30)
    dens = est.fit_predict(x, times)
    assert dens.shape == (180,) and np.isfinite(dens).all()
    assert est.pre_transformation_std is not None and len(est.losses) == 20


def test_run_advi_needs_the_batched_loss(mellon):
    with pytest.raises(NotImplementedError):
        mellon.inference.run_advi(lambda z: float(np.sum(np.square(z))), np.zeros(4))
