"""Ownership of the library's internal device and pinned memory (-m gpu): whatever a call or a handle allocated through the
caching allocator is handed back when the call returns / the handle is closed, on the ordinary paths and on the early returns
the suite already provokes (factorisation verdicts, declined and reverted rebuilds).  Seen through mln_diag_alloc_stats.

Protocol of every case: the scenario runs twice as warm-up (the context's grow-only scratch, the pooled events and the caches
reach their size), the books are read, and after each of three more runs the live device blocks, their bytes and the live
pinned blocks equal that reading exactly."""
import gc

import numpy as np
import pytest

from oracle import mellon_oracle as mo

pytestmark = pytest.mark.gpu

SETTLED = ("live_blocks", "live_bytes", "live_pinned_blocks")


@pytest.fixture(scope="module")
def mellon():
    import mellon_amd
    return mellon_amd


@pytest.fixture(scope="module")
def ctx():
    from mellon_amd import _lib
    return _lib.default_context()


def _books():
    from mellon_amd import _lib
    gc.collect()
    return _lib.alloc_stats()


def assert_settled(scenario):
    for _ in range(2):
        scenario()
    s0 = _books()
    for rep in range(3):
        scenario()
        s = _books()
        assert {k: s[k] for k in SETTLED} == {k: s0[k] for k in SETTLED}, (rep, s0, s)


def test_alloc_stats_count_the_library_s_own_blocks_only(ctx):
    """No kernel launched: a DeviceArray (mln_malloc) is not on the books; a fit handle is, until it is closed; returning the
    cache to the driver empties the cache and leaves the blocks in use alone."""
    from mellon_amd import _lib, cov
    keys = ("live_blocks", "live_bytes", "live_pinned_blocks", "cached_bytes", "driver_allocs")
    s0 = _books()
    assert set(s0) == set(keys)
    a = ctx.empty((1000, 7))
    assert _books() == s0
    a.free()
    assert _books() == s0
    rng = np.random.default_rng(0)
    x = rng.normal(size=(300, 3))
    fit = ctx.fit_prepare(cov.Matern52(1.0).lower(3), x, x[:32], 1e-6)
    s1 = _books()
    assert s1["live_blocks"] > s0["live_blocks"] and s1["live_bytes"] > s0["live_bytes"]
    _lib.release_cached_memory()
    s2 = _books()
    assert s2["cached_bytes"] == 0 and s2["live_blocks"] == s1["live_blocks"] and s2["live_bytes"] == s1["live_bytes"]
    fit.close()
    s3 = _books()
    assert s3["live_blocks"] < s1["live_blocks"] and s3["live_bytes"] < s1["live_bytes"]    # (the context keeps its scratch)
    assert s3["live_pinned_blocks"] == s0["live_pinned_blocks"]


def test_default_estimator_fit_and_predict(mellon):
    """Everything left to the estimator: nearest-neighbour distances, k-means landmarks, length scale, fit, predictor."""
    x = mo.gaussian_mixture(6000, 6, seed=41)

    def scenario():
        est = mellon.DensityEstimator(n_landmarks=150)
        dens = est.fit_predict(x)
        pred = est.predict(x[:500])
        assert np.isfinite(dens).all() and np.isfinite(np.asarray(pred)).all()
        est._fit.close()
        del est

    assert_settled(scenario)


@pytest.fixture(scope="module")
def handle_problem():
    n, d, m = 4000, 6, 300
    x = mo.gaussian_mixture(n, d, seed=n + m)
    nn = mo.exact_nn_distances(x)
    ls = mo.compute_ls(nn)
    mu = mo.compute_mu(nn, d)
    xu = x[np.sort(np.random.default_rng(n + m).choice(n, m, replace=False))]
    V, Vdr = mo.nn_likelihood_constants(nn, d)
    return x, xu, ls, mu, V, Vdr, mo.mle(nn, d) - mu


@pytest.mark.parametrize("implicit", [True, False])
def test_bare_handle_build_drop_rebuild_solve(ctx, handle_problem, implicit):
    """implicit: R, R^-1, P; explicit: the stacked operators Q1 / Q2.  The second build drops the first factor."""
    from mellon_amd import cov
    x, xu, ls, mu, V, Vdr, target = handle_problem
    desc = cov.Matern52(ls).lower(x.shape[1])

    def scenario():
        fit = ctx.fit_prepare(desc, x, xu, 1e-6, implicit=implicit)
        fit.set_likelihood(V, Vdr, mu)
        fit.precond_build(4, 0, force=True)
        fit.precond_build(1, 0, force=True)
        z0 = fit.ridge_init(target)
        z, loss, _, _, _ = fit.map_solve(z0)
        f = fit.transform(z, mu)
        assert np.isfinite(loss) and np.isfinite(f).all()
        fit.close()

    assert_settled(scenario)


@pytest.fixture(scope="module")
def rebuild_problem():
    from sklearn.cluster import k_means
    n, d, m = 40_000, 10, 300
    x = mo.gaussian_mixture(n, d, seed=13)
    nn = mo.exact_nn_distances(x)
    lm = np.ascontiguousarray(k_means(x[:8000], m, n_init=1, random_state=42)[0])
    return x, nn, lm


KNOBS = ("MELLON_AMD_MIXED", "MELLON_AMD_SUBSAMPLE", "MELLON_AMD_REBUILD", "MELLON_AMD_REBUILD_RANGE", "MELLON_AMD_REVERT_AFTER",
         "MELLON_AMD_MAX_REBUILDS")


@pytest.mark.parametrize("knobs", [{"MELLON_AMD_REBUILD_RANGE": "0"},                                   # every rebuild declines
                                   {"MELLON_AMD_REVERT_AFTER": "1", "MELLON_AMD_MAX_REBUILDS": "1"}])   # the rebuilt one fails its trial
def test_rebuild_decline_and_revert(mellon, monkeypatch, rebuild_problem, knobs):
    from mellon_amd import distributed
    x, nn, lm = rebuild_problem
    n = x.shape[0]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MELLON_AMD_REBUILD", "1")
    monkeypatch.setenv("MELLON_AMD_MIXED", "0")
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    revert = "MELLON_AMD_REVERT_AFTER" in knobs

    def check_branch(st):
        if revert:
            assert int(st["precond_reverts"]) == 1
        else:
            assert int(st["precond_rebuilds_declined"]) >= 1

    def scenario():
        est = mellon.DensityEstimator(landmarks=lm, nn_distances=nn, check_rank=False)
        dens = est.fit_predict(x)
        check_branch(est._fit.stage_times())
        assert np.isfinite(dens).all()
        est._fit.close()
        del est

    assert_settled(scenario)
    if not revert:
        return

    def body(comm):
        lo, hi = distributed.shard_bounds(n, comm.world_size, comm.rank)
        e = mellon.DensityEstimator(landmarks=lm, nn_distances=nn[lo:hi], check_rank=False)
        dens = e.fit_predict(np.ascontiguousarray(x[lo:hi]))
        reverts = int(e._fit.stage_times()["precond_reverts"])
        e._fit.close()
        return bool(np.isfinite(dens).all()), reverts

    def sharded():      # the loopback all-reduce's temporaries and the per-rank contexts
        parts = distributed.run_loopback(3, body)
        assert all(p[0] for p in parts) and len({p[1] for p in parts}) == 1

    assert_settled(sharded)


def test_factorisation_verdicts_leave_nothing_behind(ctx):
    """Host-side verdicts of a Cholesky factorisation, not device faults: cov(xu, xu) + jitter I with a negated kernel.
    The explicit route fails inside fit_prepare; the implicit (deferred) route fails in the preconditioner's batched chain,
    on every retry, and in the direct request for Lp."""
    from mellon_amd import cov
    rng = np.random.default_rng(0)
    x = rng.normal(size=(400, 3))
    bad = (cov.Matern52(1.0) * -1.0).lower(3)

    def scenario():
        with pytest.raises(ValueError):
            ctx.fit_prepare(bad, x, x[:64], 1e-6)
        fit = ctx.fit_prepare(bad, x, x[:64], 1e-6, implicit=True)
        with pytest.raises(ValueError):
            fit.precond_build(1, 0, force=True)
        for _ in range(2):
            try:
                fit.precond_build(1, 0, force=True)
            except ValueError:
                pass
        try:
            fit.Lp()
        except ValueError:
            pass
        fit.close()

    assert_settled(scenario)


def test_stand_alone_operators(ctx):
    from mellon_amd import cov
    rng = np.random.default_rng(5)
    xk = mo.gaussian_mixture(20_000, 10, seed=5)
    A = rng.normal(size=(200, 200))
    A = A @ A.T
    x = rng.normal(size=(3000, 4))
    xu = x[:128]
    one = cov.Matern52(1.3).lower(4)
    two = (cov.Matern52(1.1, active_dims=[0, 1]) * cov.ExpQuad(0.9, active_dims=[2, 3])).lower(4)
    w = rng.normal(size=128)
    y = rng.normal(size=(3000, 3))

    def scenario():
        c = ctx.kmeans(xk, 256, seed=42)
        lam, vec = ctx.eigh(A)
        G = ctx.kernel_gram(one, x, xu)
        g = ctx.predict_gradient(two, x[:700], xu, w)
        W = ctx.sparse_solve(one, x, xu, y, 0.1, 0.5, 1e-6)
        for r in (c, lam, vec, G, g, W):
            assert np.isfinite(np.asarray(r)).all()

    assert_settled(scenario)
