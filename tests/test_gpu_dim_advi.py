"""DimensionalityEstimator(optimizer="advi") on a real MI355X (-m gpu): the batched dimensionality objective
(mln_dim_objective_batch) against single passes on the same handle and against the NumPy restatement
(tests/dim_restatement.py), sharded against unsharded, run_advi against the restatement of the ADVI loop
(tests/dim_advi_restatement.py) with the same draws, and the estimator surface of the reference's
tests/test_dimensionality_estimator.py:63-112 with the real optimiser.

Tolerances: the batched objective is held to what tests/test_gpu_advi.py holds mln_objective_batch to, the same MFMA
reduction: loss 1e-11 relative, gradient 1e-8 of the sample's largest entry.  The trajectory's bound is computed in its
test from the restatement's own sensitivity to gradient noise of that size (Adam divides by sqrt(v): where a mean
gradient is near zero, rounding is amplified)."""
import json

import numpy as np
import pytest

import dim_advi_restatement as dar
import dim_restatement as dr
from oracle import mellon_oracle as mo

pytestmark = pytest.mark.gpu

C = 32                      # samples per chunk of mln_dim_objective_batch
MU_DIM, MU_DENS = 0.3, 1.1


@pytest.fixture(scope="module")
def mellon():
    import mellon_amd
    return mellon_amd


@pytest.fixture(scope="module")
def ctx():
    from mellon_amd import _lib
    return _lib.default_context()


@pytest.fixture(scope="module")
def small_x():
    # the reference's tests/test_dimensionality_estimator.py: n = 100, d = 2, correlated normal
    rng = np.random.default_rng(535)
    A = rng.uniform(size=(2, 2))
    return rng.multivariate_normal(np.ones(2), A.T @ A, size=100)


def relmax(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _check_batch(fit, Z, L=None, ell=None, tag=""):
    """dim_objective_batch(Z) against len(Z) single passes on the same handle and (given L) the restatement; identical
    bits twice; the flat form of Z gives the flat form of the same gradient."""
    S, m = Z.shape[0], Z.shape[2]
    loss, grad = fit.dim_objective_batch(Z)
    assert loss.shape == (S,) and grad.shape == Z.shape
    loss2, grad2 = fit.dim_objective_batch(Z.reshape(S, 2 * m))
    assert grad2.shape == (S, 2 * m)
    assert np.array_equal(loss, loss2) and np.array_equal(grad, grad2.reshape(Z.shape))
    assert np.isfinite(loss).all() and np.isfinite(grad).all()
    singles = [fit.dim_objective(z) for z in Z]
    l1 = np.array([s[0] for s in singles])
    g1 = np.stack([s[1] for s in singles])
    e_loss = np.abs(loss - l1) / np.abs(l1)
    e_grad = max(relmax(grad[s], g1[s]) for s in range(S))
    print(f"{tag} S={S} m={m}: vs single passes loss {e_loss.max():.2e} grad {e_grad:.2e}", end="")
    assert e_loss.max() < 1e-11 and e_grad < 1e-8
    if L is not None:
        ref_l = np.array([dr.dim_loss(z, L, ell, MU_DIM, MU_DENS) for z in Z])
        ref_g = np.stack([dr.dim_grad_hess(z, L, ell, MU_DIM, MU_DENS)[0] for z in Z])
        assert np.isfinite(ref_l).all() and np.isfinite(ref_g).all()
        o_loss = (np.abs(loss - ref_l) / np.abs(ref_l)).max()
        o_grad = max(relmax(grad[s], ref_g[s]) for s in range(S))
        print(f"; vs restatement loss {o_loss:.2e} grad {o_grad:.2e}", end="")
        assert o_loss < 1e-11 and o_grad < 1e-8
    print()


def _from_L_case(ctx, n, m, k, seed):
    from mellon_amd import _lib
    rng = np.random.default_rng(seed)
    L = rng.normal(size=(n, m)) * (0.5 / np.sqrt(m))
    ell = dr.ell_of(np.abs(rng.normal(size=(n, k))) + 0.05)
    fit = _lib.Fit.from_L(ctx, L)
    fit.set_dim_likelihood(ell, MU_DIM, MU_DENS)
    return rng, L, ell, fit


# ---- 1. the batched objective -------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,S,k", [(1, 4, 1, 1), (3, 255, 2, 10), (16, 257, 16, 10), (17, 1501, 33, 64), (100, 777, 40, 10),
                                     (1000, 1501, 15, 3), (5000, 777, 40, 10), (5120, 300, 5, 10)])
def test_batch_shapes(ctx, m, n, S, k):
    """A single partial row tile, the row tail, the column tail of the backward tile, the maximum width, k = 1 and 64."""
    rng, L, ell, fit = _from_L_case(ctx, n, m, k, seed=1000 * m + S)
    Z = rng.normal(size=(S, 2, m)) * 0.2
    _check_batch(fit, Z, L, ell, tag="from_L")
    fit.close()


@pytest.fixture(scope="module")
def count_case(ctx):
    rng, L, ell, fit = _from_L_case(ctx, 2049, 100, 10, seed=5)
    yield L, ell, fit
    fit.close()


@pytest.mark.parametrize("S", [1, 15, 16, 17, C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1, 40, 100])
def test_batch_sample_counts(count_case, S):
    """Every chunking of S (one to four launches, every padding of the last one) on one factor."""
    L, ell, fit = count_case
    Z = np.random.default_rng(S).normal(size=(S, 2, 100)) * 0.2
    _check_batch(fit, Z, L, ell, tag="from_L")


def _fit_case(kind, n, m, d=3, seed=0):
    """The handle layouts of tests/test_gpu_dimensionality.py (re-created)."""
    from mellon_amd import _lib, cov
    from mellon_amd.decomposition import _full_decomposition_low_rank, _modified_low_rank
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, d))
    k = cov.Matern52(1.3)
    c = _lib.default_context()
    if kind == "full":
        fit = c.fit_prepare(k.lower(d), x, None, 1e-6)
    elif kind == "sparse_cholesky":
        fit = c.fit_prepare(k.lower(d), x, x[rng.choice(n, m, replace=False)], 1e-6)
    elif kind == "implicit":
        fit = c.fit_prepare(k.lower(d), x, x[rng.choice(n, m, replace=False)], 1e-6, implicit=True)
    elif kind == "full_nystroem":
        fit = _full_decomposition_low_rank(x, k, rank=0.999, jitter=1e-6).fit
    else:
        fit = _modified_low_rank(x, k, x[rng.choice(n, m, replace=False)], rank=0.999, jitter=1e-6).fit
    return x, fit


@pytest.mark.parametrize("kind,n,m", [("sparse_cholesky", 3001, 130), ("implicit", 3001, 130), ("full", 300, None),
                                      ("full_nystroem", 400, None), ("sparse_nystroem", 1500, 200)])
def test_batch_handle_kinds(kind, n, m):
    x, fit = _fit_case(kind, n, m)
    rng = np.random.default_rng(1)
    L = fit.L()
    ell = dr.ell_of(np.abs(rng.normal(size=(fit.n, 10))) + 0.05)
    fit.set_dim_likelihood(ell, MU_DIM, MU_DENS)
    for S in (40, 17):
        Z = rng.normal(size=(S, 2, fit.m)) * 0.1
        _check_batch(fit, Z, L, ell, tag=kind)


def test_batch_argument_errors(ctx):
    from mellon_amd import _lib
    L = np.random.default_rng(0).normal(size=(50, 7))
    fit = _lib.Fit.from_L(ctx, L)
    with pytest.raises((_lib.MellonHipError, ValueError)):
        fit.dim_objective_batch(np.zeros((3, 2, 7)))          # no likelihood yet
    fit.set_dim_likelihood(np.zeros((50, 4)), 0.0, 0.0)
    for shape in ((3, 2, 8), (3, 7), (3, 15), (3, 1, 14), (2, 7), (3, 2, 7, 1)):
        with pytest.raises(ValueError):
            fit.dim_objective_batch(np.zeros(shape))
    with pytest.raises(ValueError):
        fit.dim_objective_batch(np.zeros((0, 2, 7)))
    with pytest.raises(ValueError):
        fit.dim_objective_batch(np.zeros((0, 14)))
    loss, grad = fit.dim_objective_batch(np.zeros((3, 14)))
    assert loss.shape == (3,) and grad.shape == (3, 14)
    fit.close()


# ---- 2. sharded ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ranks", [2, 3])
@pytest.mark.parametrize("implicit", [False, True])
def test_batch_sharded(ctx, n_ranks, implicit):
    """Uneven shards on loopback thread-ranks: one all-reduce of the losses and the gradient block, prior terms once."""
    from mellon_amd import cov, distributed
    n, d, m = 3001, 3, 130
    rng = np.random.default_rng(77)
    x = rng.normal(size=(n, d))
    xu = x[rng.choice(n, m, replace=False)]
    desc = cov.Matern52(1.3).lower(d)
    ell = dr.ell_of(np.abs(rng.normal(size=(n, 10))) + 0.05)
    Z = 0.1 * rng.normal(size=(40, 2, m))
    one = ctx.fit_prepare(desc, x, xu, 1e-6, implicit=implicit)
    one.set_dim_likelihood(ell, MU_DIM, MU_DENS)
    loss1, grad1 = one.dim_objective_batch(Z)
    cuts = [0] + [int(n * f) for f in ((0.37,) if n_ranks == 2 else (0.2, 0.71))] + [n]

    def body(comm):
        lo, hi = cuts[comm.rank], cuts[comm.rank + 1]
        f = comm.ctx.fit_prepare(desc, np.ascontiguousarray(x[lo:hi]), xu, 1e-6, implicit=implicit)
        f.set_dim_likelihood(ell[lo:hi], MU_DIM, MU_DENS)
        out = f.dim_objective_batch(Z)
        f.close()
        return out

    res = distributed.run_loopback(n_ranks, body)
    for loss, grad in res:
        assert np.array_equal(loss, res[0][0]) and np.array_equal(grad, res[0][1])     # same bits on every rank
        e_loss = (np.abs(loss - loss1) / np.abs(loss1)).max()
        e_grad = max(relmax(grad[s], grad1[s]) for s in range(len(Z)))
        print(f"{n_ranks} ranks implicit={implicit}: loss {e_loss:.2e} grad {e_grad:.2e}")
        assert e_loss < 1e-11 and e_grad < 1e-8


# ---- 3. run_advi against the restatement ----------------------------------------------------------------------------
N_ITER, N_DRAWS = 20, 40


@pytest.fixture(scope="module")
def real_problem(ctx):
    """300 cells in 3 dimensions, 40 landmarks, k = 10; length scale and density mean by the oracle's rules, the start from
    the restatement's Ridge.  Holds the restatement's clean trajectory (with its parameters after every step) and the
    trajectory under gradient noise of the device's tolerance."""
    from mellon_amd import cov, inference
    rng = np.random.default_rng(0)
    x = rng.normal(size=(300, 3))
    distances = dar.knn_distances(x, 10)
    nn = np.ascontiguousarray(distances[:, 0])
    d = dr.local_dimensionality(x)
    ls, mu_dim, mu_dens = mo.compute_ls(nn), 0.0, mo.compute_mu(nn, d)
    xu = x[rng.choice(300, size=40, replace=False)]
    fit = ctx.fit_prepare(cov.Matern52(ls).lower(3), x, xu, 1e-6)
    L = fit.L()
    ell = dr.ell_of(distances)
    z0 = dr.initial_dimensionalities(L, d, mu_dim, nn, mu_dens)
    args = (L, ell, mu_dim, mu_dens)
    history = []
    clean = dar.run_advi(z0, *args, n_iter=N_ITER, nsamples=N_DRAWS, history=history)
    noisy = dar.run_advi(z0, *args, n_iter=N_ITER, nsamples=N_DRAWS, noise=np.random.default_rng(2024))
    transform = inference.compute_dimensionality_transform(mu_dim, mu_dens, L)
    loss_func = inference.compute_dimensionality_loss_func(distances, transform, 2)
    return dict(args=args, z0=z0, clean=clean, noisy=noisy, history=history, loss_func=loss_func)


@pytest.mark.parametrize("step", [0, 1, 5, 19])
def test_teacher_forced_elbo(real_problem, step):
    """At the restatement's parameters after `step`, with the draws of the next step: the device's ELBO value and both
    gradient leaves against the restatement's."""
    p = real_problem
    mean, log_std = p["history"][step]
    eps = dar.advi_draws(step + 1, N_DRAWS, mean.size)
    want = dar.elbo_value_and_grad(mean, log_std, eps, *p["args"])
    got = dar.elbo_value_and_grad(mean, log_std, eps, *p["args"], batch=p["loss_func"].value_and_grad_batch)
    e_val = abs(got[0] - want[0]) / abs(want[0])
    e_mean, e_std = relmax(got[1], want[1]), relmax(got[2], want[2])
    print(f"after step {step}: value {e_val:.2e} d/dmean {e_mean:.2e} d/dlog_std {e_std:.2e}")
    assert np.isfinite(want[0]) and got[1].shape == (2, 40) and got[2].shape == (2, 40)
    assert e_val < 1e-11 and e_mean < 1e-8 and e_std < 1e-8


def test_run_advi_trajectory(real_problem):
    """20 steps x 40 draws on the device loss against the restatement's trajectory.  The bound is ten times what gradient
    noise of 1e-8 (the device's gradient tolerance) does to the restatement itself; the factor covers the noise's seed."""
    from mellon_amd import inference
    p = real_problem
    loss_func = p["loss_func"]
    before = loss_func.n_eval
    got = inference.run_advi(loss_func, p["z0"], n_iter=N_ITER, nsamples=N_DRAWS)
    assert loss_func.n_eval - before == N_ITER * N_DRAWS
    clean, noisy = p["clean"], p["noisy"]

    def errors(mean, std, losses):
        return (np.abs(mean - clean[0]).max(), np.abs(std / clean[1] - 1).max(),
                np.abs(np.asarray(losses) / clean[2] - 1).max())

    bound = [10 * e for e in errors(*noisy)]
    err = errors(got.pre_transformation, got.pre_transformation_std, got.losses)
    print(f"|dmean| {err[0]:.2e} (bound {bound[0]:.2e}) rel dstd {err[1]:.2e} (bound {bound[1]:.2e}) "
          f"rel dlosses {err[2]:.2e} (bound {bound[2]:.2e})")
    assert got.pre_transformation.shape == (2, 40) and got.pre_transformation_std.shape == (2, 40)
    assert len(got.losses) == N_ITER and np.isfinite(got.losses).all()
    assert all(b > 0 for b in bound)
    assert err[0] <= bound[0] and err[1] <= bound[1] and err[2] <= bound[2]


# ---- 4. the estimator -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rank,n_landmarks", [(1.0, 0), (0.99, 0), (1.0, 10), (0.99, 80)])
def test_dimensionality_estimator_advi_uncertainty(mellon, small_x, tmp_path, rank, n_landmarks):
    n = small_x.shape[0]
    est = mellon.DimensionalityEstimator(rank=rank, n_landmarks=n_landmarks, optimizer="advi",
                                         predictor_with_uncertainty=True, n_iter=30)
    est.fit(small_x)
    m = est.pre_transformation.shape[1]
    assert est.pre_transformation.shape == (2, m) and est.pre_transformation_std.shape == (2, m)
    assert np.all(est.pre_transformation_std > 0)
    assert len(est.losses) == 30 and np.isfinite(est.losses).all()
    assert est.loss_func.n_eval == 30 * 40
    p = est.predict
    v, lv = p(small_x), p(small_x, logscale=True)
    assert np.isfinite(v).all() and np.allclose(v, np.exp(lv))
    assert p.covariance(small_x).shape == (n,)
    assert p.mean_covariance(small_x).shape == (n,)
    unc = p.uncertainty(small_x)
    assert unc.shape == (n,)
    path = str(tmp_path / f"dim_advi_{n_landmarks}_{rank}.json")
    p.to_json(path)
    again = mellon.Predictor.from_json(path)
    assert np.allclose(again(small_x), v) and np.allclose(again.uncertainty(small_x), unc)
    json.loads(p.to_json())


def test_dimensionality_estimator_advi_without_uncertainty(mellon, small_x):
    est = mellon.DimensionalityEstimator(optimizer="advi", n_iter=25)
    dim = est.fit_predict(small_x, build_predict=True)
    assert dim.shape == (100,) and np.isfinite(dim).all()
    m = est.pre_transformation.shape[1]
    assert est.pre_transformation_std is not None and est.pre_transformation_std.shape == (2, m)
    assert len(est.losses) == 25
    with pytest.raises(ValueError):                      # as for the density estimator: the predictor holds no covariance
        est.predict.uncertainty(small_x)


def test_prepared_estimator_is_not_switched_to_advi(mellon, small_x):
    """The one remaining limit: run_inference(..., "advi") on an estimator constructed with another optimiser."""
    other = mellon.DimensionalityEstimator()
    loss_func, start = other.prepare_inference(small_x)
    with pytest.raises(NotImplementedError, match='optimizer="advi"'):
        other.run_inference(loss_func, start, "advi")
    assert other.optimizer == "L-BFGS-B"
    est = mellon.DimensionalityEstimator(optimizer="advi", n_iter=5)
    loss_func, start = est.prepare_inference(small_x)
    assert est.run_inference(loss_func, start, "advi").shape == start.shape and len(est.losses) == 5


def test_dimensionality_estimator_advi_sharded(mellon, small_x):
    """Two loopback ranks: finite rows on each, one optimiser path (the same bits) on both."""
    from mellon_amd import distributed
    cut = 37

    def body(comm):
        xs = np.ascontiguousarray(small_x[:cut] if comm.rank == 0 else small_x[cut:])
        est = mellon.DimensionalityEstimator(optimizer="advi", n_iter=10, n_landmarks=20)
        dim = est.fit_predict(xs)
        return dim, est.pre_transformation, est.pre_transformation_std, est.losses

    res = distributed.run_loopback(2, body)
    assert res[0][0].shape == (cut,) and res[1][0].shape == (100 - cut,)
    for dim, z, std, losses in res:
        assert np.isfinite(dim).all() and z.shape == std.shape and z.shape[0] == 2 and len(losses) == 10
        assert np.array_equal(z, res[0][1]) and np.array_equal(std, res[0][2])
