"""FunctionEstimator on cells sharded across ranks, on ONE GPU: N thread-ranks joined by the library's loopback
communicator (distributed.run_loopback) run the real sharded code -- per-rank rows of A, the all-reduced A A^T and
A (y - mu), the replicated m x m factor work, the global decisions over the host communicator -- and must reproduce the
single-rank fit; two PROCESSES over the host-staged transport do the same for the scalar-sigma case.

Base workload (tests/function_shard_workload.py): n = 2399 cells (uneven shards), d = 5, p = 3 smooth targets plus
noise, 150 given landmarks, sigma = 0.3; 2 and 3 ranks; the sharded result is the concatenation of the ranks' rows.

`TOL`.  What differs between one rank and N is the order of the sums in A A^T and A (y - mu), amplified by the
conditioning of A A^T / sigma^2 + I.  Measured on the CPU with the oracle's landmark conditional in two steps
(tools/function_shard_tol.py, which never imports the sharded code): the two sums formed once over all rows and shard by
shard in rank order for 2, 3 and 4 shards; the largest change of the predictions (training cells and 64 held-out
points) relative to the largest absolute prediction, over 5 data seeds, is 9.455683e-13 (per seed 2.678197e-13,
2.506680e-13, 7.001736e-13, 4.946896e-13, 9.455683e-13).  TOL = 16 x that = 1.512909e-11, the factor for the device's
different blocking inside each partial sum.  Every comparison prints its figure before it asserts.

Observed on one MI355X (2 and 3 thread-ranks): predictions within 3.3e-13 (scalar sigma), 5.4e-13 (per output), 3.5e-13
(per cell and output), 2.7e-13 (per cell), 2.1e-12 (CSR, p = 40), 7.5e-13 (40 levels, spectral; its leverage 4.1e-14),
`Cs` within 1.6e-15, `L` equal.  With `obs_variance=True`: the B^T B leverage equal bit for bit, `_corrected_r2` within
9.0e-13, `variance_weights` 2.4e-12, `obs_variance(X)` 1.4e-12.  That leverage inverts M = sigma^2 K_uu + B^T B +
jitter I (conditional.py:660-685), whose condition number here is 7e10 .. 1.3e11: with an all-reduce of per-rank Grams
it missed TOL by three orders of magnitude (leverage 2.0e-8 .. 8.4e-8, residuals up to 1.3e-8, variance weights up to
9.4e-9 -- the ORACLE's own leverage moves by 5.7e-9 .. 1.6e-8 when its B^T B is summed shard by shard, second figure of
tools/function_shard_tol.py), which is why B^T B is formed in the single-rank order on every rank
(conditional._kernel_gram_all_ranks).
"""
import json
import os
import socket
import subprocess
import sys
import threading

import numpy as np
import pytest

from function_shard_workload import N_HELD_OUT, SIGMA, make_workload

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TOL = 16 * 9.455683e-13


# ---- running ranks ---------------------------------------------------------------------------------------------------
def _run_ranks(n_ranks, body, deadline=300.0):
    """distributed.run_loopback under a deadline: a rank left waiting in a collective fails the test instead of
    blocking it.  (Bodies that expect errors return them, so no rank is ever released by another one's failure.)"""
    from mellon_amd import distributed
    box = {}

    def run():
        try:
            box["out"] = distributed.run_loopback(n_ranks, body)
        except BaseException as e:      # noqa: BLE001 -- re-raised on the test's thread
            box["error"] = e

    t = threading.Thread(target=run, daemon=True)
    t.start()
    t.join(deadline)
    assert not t.is_alive(), "a rank is still waiting in a collective"
    if "error" in box:
        raise box["error"]
    return box["out"]


def _rows(a, lo, hi):
    """Rows [lo, hi) of dense or SciPy-sparse targets / of a sigma that has one entry per cell."""
    return a[lo:hi] if hasattr(a, "tocsr") else np.ascontiguousarray(a[lo:hi])


def _state(est, x_new, train):
    p = est.predict
    return dict(train=train, new=p(x_new), weights=p.weights, n_obs=p.n_obs, ls=est.ls, gp_type=est.gp_type,
                n_landmarks=est.n_landmarks, landmarks=np.asarray(est.landmarks), x_rows=est.x.shape[0])


def _one_openmp_thread():
    """scikit-learn's k-means adds the partial sums of its threads in completion order: two runs of the SAME call differ
    in the last bit unless the calling thread's OpenMP pool is held to one thread (a per-thread setting)."""
    from threadpoolctl import threadpool_limits
    return threadpool_limits(limits=1, user_api="openmp")


def _fit_one(x, y, x_new, make_est, extra=None):
    est = make_est(0, x.shape[0])
    with _one_openmp_thread():
        out = _state(est, x_new, est.fit_predict(x, y))
    if extra is not None:
        out.update(extra(est, None, 0, x.shape[0]))
    return out


def _fit_sharded(n_ranks, x, y, x_new, make_est, extra=None):
    from mellon_amd import distributed

    def body(comm):
        lo, hi = distributed.shard_bounds(x.shape[0], comm.world_size, comm.rank)
        est = make_est(lo, hi)
        with _one_openmp_thread():
            out = _state(est, x_new, est.fit_predict(np.ascontiguousarray(x[lo:hi]), _rows(y, lo, hi)))
        assert est.x.shape[0] == hi - lo and est.y.shape[0] == hi - lo          # est.x / est.y stay the shard
        if extra is not None:
            out.update(extra(est, comm, lo, hi))
        return out

    return _run_ranks(n_ranks, body)


def _rel(got, want, scale, what):
    err = float(np.abs(np.asarray(got) - np.asarray(want)).max() / scale)
    print(f"{what}: {err:.3e} (tol {TOL:.3e})")
    return err


def _check_against_one_rank(res, one, what):
    """Replicated weights bit-identical across ranks; predictions (training cells: concatenated rows; held-out points:
    every rank's copy) within TOL of the single-rank fit, relative to the largest absolute prediction."""
    assert all(np.array_equal(r["weights"], res[0]["weights"]) for r in res), "weights differ between ranks"
    assert all(np.array_equal(r["new"], res[0]["new"]) for r in res)
    train = np.concatenate([r["train"] for r in res], axis=0)
    assert train.shape == one["train"].shape
    scale = max(np.abs(one["train"]).max(), np.abs(one["new"]).max())
    errs = [_rel(train, one["train"], scale, f"{what}: training cells"), _rel(res[0]["new"], one["new"], scale, f"{what}: held-out")]
    assert max(errs) <= TOL, errs


@pytest.fixture(scope="module")
def base():
    return make_workload()


# ---- 1. equality with one rank under each noise model ----------------------------------------------------------------
def _noise_models(n, p):
    rng = np.random.default_rng(17)
    per_output = np.array([0.2, 0.3, 0.5])[:p]
    per_entry = 0.2 + 0.3 * rng.uniform(size=(n, p))
    return {"scalar": lambda lo, hi: SIGMA,
            "per_output": lambda lo, hi: per_output,
            "per_output_row": lambda lo, hi: per_output[None, :],
            "per_cell_and_output": lambda lo, hi: np.ascontiguousarray(per_entry[lo:hi])}


@pytest.fixture(scope="module")
def one_rank_by_noise(base):
    import mellon_amd
    x, y, lm, x_new = base
    return {name: _fit_one(x, y, x_new, lambda lo, hi: mellon_amd.FunctionEstimator(landmarks=lm, sigma=sig(lo, hi)))
            for name, sig in _noise_models(*y.shape).items()}


@pytest.mark.parametrize("n_ranks", [2, 3])
@pytest.mark.parametrize("noise", ["scalar", "per_output", "per_output_row", "per_cell_and_output"])
def test_sharded_fit_equals_one_rank(base, one_rank_by_noise, noise, n_ranks):
    import mellon_amd
    x, y, lm, x_new = base
    sig = _noise_models(*y.shape)[noise]
    res = _fit_sharded(n_ranks, x, y, x_new, lambda lo, hi: mellon_amd.FunctionEstimator(landmarks=lm, sigma=sig(lo, hi)))
    one = one_rank_by_noise[noise]
    assert all(r["ls"] == one["ls"] and r["gp_type"] == one["gp_type"] for r in res)
    _check_against_one_rank(res, one, f"{noise}, {n_ranks} ranks")


# ---- 2. decisions from global quantities -----------------------------------------------------------------------------
def test_decisions_heuristics_and_landmarks_are_global():
    """n = 1200 on 3 ranks with n_landmarks = 500: every shard (400 cells) is smaller than n_landmarks, so a decision on
    the local count picks the full GP.  gp_type, n_landmarks, ls and the k-means landmarks are the single-rank bits."""
    import mellon_amd
    from mellon_amd.util import GaussianProcessType
    x, y, _, x_new = make_workload(seed=8, n=1200, m=0)
    make = lambda lo, hi: mellon_amd.FunctionEstimator(n_landmarks=500, sigma=SIGMA)
    one = _fit_one(x, y, x_new, make)
    res = _fit_sharded(3, x, y, x_new, make)
    assert one["gp_type"] == GaussianProcessType.SPARSE_CHOLESKY
    for r in res:
        assert r["gp_type"] == one["gp_type"] and r["n_landmarks"] == one["n_landmarks"] == 500
        assert r["ls"] == one["ls"]
        assert np.array_equal(r["landmarks"], one["landmarks"])
        assert r["n_obs"] == 1200 and r["x_rows"] == 400
    _check_against_one_rank(res, one, "global decisions")


# ---- 3. what is refused, on every rank --------------------------------------------------------------------------------
def test_full_gp_and_input_errors_are_raised_on_every_rank():
    """n = 300 on 3 ranks.  The bodies return what they raised: nobody is released by a peer's failure, so a rank left
    in a collective would run into the deadline."""
    import mellon_amd
    from mellon_amd import distributed
    x, y, _, _ = make_workload(seed=9, n=300, m=0)

    def attempt(comm, y_of=lambda a: a, **kw):
        lo, hi = distributed.shard_bounds(300, comm.world_size, comm.rank)
        try:
            mellon_amd.FunctionEstimator(sigma=SIGMA, **kw).fit(np.ascontiguousarray(x[lo:hi]), y_of(np.ascontiguousarray(y[lo:hi])))
        except Exception as e:      # noqa: BLE001 -- the result
            return e
        return None

    def body(comm):
        short = (lambda a: a[:-1]) if comm.rank == 1 else (lambda a: a)
        return attempt(comm), attempt(comm, gp_type="full"), attempt(comm, y_of=short, n_landmarks=40), \
            attempt(comm, n_landmarks=40)

    res = _run_ranks(3, body, deadline=120.0)
    for default, full, mismatch, fine in res:
        assert isinstance(default, NotImplementedError) and "full Gaussian process of the FunctionEstimator" in str(default)
        assert isinstance(full, NotImplementedError) and "full Gaussian process of the FunctionEstimator" in str(full)
        assert isinstance(mismatch, ValueError) and str(mismatch) == str(res[0][2]) and "rank 1:" in str(mismatch)
        assert fine is None          # ... and the communicator is still usable afterwards


# ---- 4. CSR targets --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sparse_case(base):
    import scipy.sparse as sp
    x, _, lm, x_new = base
    Y = sp.random(x.shape[0], 40, density=0.10, format="csr", random_state=np.random.RandomState(4), dtype=np.float64)
    Y.data[:] = 1.0 + np.abs(Y.data) * 3.0
    levels = np.array([0.2, 0.3, 0.5])[np.arange(40) * 3 // 40]          # three runs of equal sigma
    return x, Y, lm, x_new, {"scalar": SIGMA, "per_output": levels}


@pytest.mark.parametrize("n_ranks", [2, 3])
@pytest.mark.parametrize("noise", ["scalar", "per_output"])
def test_csr_targets_sharded_by_rows(sparse_case, noise, n_ranks, monkeypatch):
    """Each rank passes Y[lo:hi] as it is; no rank forms an n x p array (CSRTargets.toarray is made to raise)."""
    import mellon_amd
    from mellon_amd import validation
    x, Y, lm, x_new, sigmas = sparse_case
    make = lambda lo, hi: mellon_amd.FunctionEstimator(landmarks=lm, sigma=sigmas[noise])
    dense = np.ascontiguousarray(Y.toarray())
    one_dense = _fit_one(x, dense, x_new, make)
    dense_sharded = _fit_sharded(n_ranks, x, dense, x_new, make)

    def no_dense(self):
        raise AssertionError("sparse targets were made dense")
    monkeypatch.setattr(validation.CSRTargets, "toarray", no_dense)
    one = _fit_one(x, Y, x_new, make)
    res = _fit_sharded(n_ranks, x, Y, x_new, make)
    _check_against_one_rank(res, one, f"CSR {noise}, {n_ranks} ranks")
    _check_against_one_rank(res, one_dense, f"CSR {noise} against dense, {n_ranks} ranks")
    if np.array_equal(one["weights"], one_dense["weights"]):       # the routes agree bit for bit on one rank: so must the shards
        assert all(np.array_equal(a["weights"], b["weights"]) and np.array_equal(a["train"], b["train"])
                   for a, b in zip(res, dense_sharded))
    else:
        _check_against_one_rank(res, dict(train=np.concatenate([r["train"] for r in dense_sharded]), new=dense_sharded[0]["new"]),
                                f"CSR {noise} against dense shards, {n_ranks} ranks")


@pytest.mark.parametrize("n_ranks", [2, 3])
def test_multi_fit_predict_with_sharded_columns(sparse_case, n_ranks):
    """Functions in rows (p x n): the columns are the cells, so each rank passes Y.T[:, lo:hi]."""
    import mellon_amd
    from mellon_amd import distributed
    x, Y, lm, x_new, _ = sparse_case
    Yt = Y.T.tocsr()
    est = mellon_amd.FunctionEstimator(landmarks=lm, sigma=SIGMA)
    one = est.multi_fit_predict(x, Yt)
    one_new = est.predict(x_new).T

    def body(comm):
        lo, hi = distributed.shard_bounds(x.shape[0], comm.world_size, comm.rank)
        e = mellon_amd.FunctionEstimator(landmarks=lm, sigma=SIGMA)
        got = e.multi_fit_predict(np.ascontiguousarray(x[lo:hi]), Yt[:, lo:hi])
        return dict(train=got.T, new=e.predict(x_new), weights=e.predict.weights)

    res = _run_ranks(n_ranks, body)
    assert one.shape == (40, x.shape[0])
    _check_against_one_rank(res, dict(train=one.T, new=one_new.T), f"multi_fit_predict, {n_ranks} ranks")


# ---- 5. more than 32 noise levels: the spectral routes ----------------------------------------------------------------
@pytest.mark.parametrize("n_ranks", [2, 3])
def test_forty_noise_levels_take_the_spectral_routes(n_ranks):
    """p = 40 distinct sigmas: mln_sparse_solve_noise goes spectral above 32 levels, and with the predictor carrying L
    (predictor_with_uncertainty) the leverage goes through mln_landmark_leverage.  leverage() is collective."""
    import mellon_amd
    x, y, lm, x_new = make_workload(p=40)
    sig = np.linspace(0.15, 0.6, 40)
    make = lambda lo, hi: mellon_amd.FunctionEstimator(landmarks=lm, sigma=sig, predictor_with_uncertainty=True)
    extra = lambda est, comm, lo, hi: dict(h=est.leverage(), L=est.predict.L)
    one = _fit_one(x, y, x_new, make, extra)
    res = _fit_sharded(n_ranks, x, y, x_new, make, extra)
    _check_against_one_rank(res, one, f"40 levels, {n_ranks} ranks")
    h = np.concatenate([r["h"] for r in res])
    assert h.shape == (x.shape[0], 40) and all(np.array_equal(r["L"], res[0]["L"]) for r in res)
    assert _rel(h, one["h"], np.abs(one["h"]).max(), f"40 levels, {n_ranks} ranks: leverage") <= TOL


# ---- 6. obs_variance and predictor_with_uncertainty -------------------------------------------------------------------
def _variance_extra(x_new):
    def extra(est, comm, lo, hi):
        p = est.predict
        out = dict(cr2=p._corrected_r2, vw=p.variance_weights, L=p.L, Cs=getattr(p, "Cs", None), W=getattr(p, "W", None))
        if comm is None or comm.rank == 0:
            # replicated state only: ONE rank calls these, the others are already waiting in leverage() below
            out["solo"] = {}
            for name, call in (("covariance", lambda: p.covariance(x_new, noise_free=True)),
                               ("uncertainty", lambda: p.uncertainty(x_new)),
                               ("obs_variance", lambda: p.obs_variance(x_new)),
                               ("get_obs_variance", lambda: est.get_obs_variance(x_new))):
                try:
                    out["solo"][name] = call()
                except ValueError as e:       # (no W without parameter uncertainty: the same refusal as on one rank)
                    out["solo"][name] = type(e).__name__
        out["h"] = est.leverage()                                    # collective: every rank, its rows
        out["loo_cached"] = est.loo_residuals_squared()               # the cached HC3 residuals of the fit
        out["loo"] = est.loo_residuals_squared(est.x, est.y)          # collective
        return out
    return extra


_VARIANCE_RUNS = {}


def _variance_runs(base, noise, n_ranks):
    """(single-rank, sharded) state of an obs_variance=True, predictor_with_uncertainty=True fit: computed once per
    case and shared by the two tests below, never modified."""
    import mellon_amd
    if (noise, n_ranks) not in _VARIANCE_RUNS:
        x, y, lm, x_new = base
        sig = _noise_models(*y.shape)[noise]
        make = lambda lo, hi: mellon_amd.FunctionEstimator(landmarks=lm, sigma=sig(lo, hi), obs_variance=True,
                                                          predictor_with_uncertainty=True)
        if ("one", noise) not in _VARIANCE_RUNS:
            _VARIANCE_RUNS["one", noise] = _fit_one(x, y, x_new, make, _variance_extra(x_new))
        _VARIANCE_RUNS[noise, n_ranks] = _fit_sharded(n_ranks, x, y, x_new, make, _variance_extra(x_new))
    return _VARIANCE_RUNS["one", noise], _VARIANCE_RUNS[noise, n_ranks]


@pytest.mark.parametrize("n_ranks", [2, 3])
@pytest.mark.parametrize("noise", ["scalar", "per_output"])
def test_uncertainty_state_and_who_has_to_call(base, noise, n_ranks):
    """The fit itself, `L`, `Cs` and `W` within TOL and replicated bit for bit (`variance_weights` too); covariance,
    uncertainty and obs_variance answered by rank 0 ALONE while the other ranks are already inside leverage();
    leverage() and loo_residuals_squared() answered with this rank's rows when all ranks call."""
    one, res = _variance_runs(base, noise, n_ranks)
    what = f"uncertainty {noise}, {n_ranks} ranks"
    _check_against_one_rank(res, one, what)
    errs = [0.0]
    for key in ("vw", "L", "Cs", "W"):
        if one[key] is None:
            assert all(r[key] is None for r in res)
            continue
        assert all(np.array_equal(r[key], res[0][key]) for r in res), key
        if key != "vw":
            errs.append(_rel(res[0][key], one[key], np.abs(one[key]).max(), f"{what}: {key}"))
    for key in ("cr2", "h", "loo", "loo_cached"):       # sharded: this rank's rows
        assert np.concatenate([r[key] for r in res], axis=0).shape == one[key].shape
    assert all(np.array_equal(r["loo_cached"], r["cr2"]) for r in res)
    solo = res[0]["solo"]
    assert all("solo" not in r for r in res[1:]) and set(solo) == set(one["solo"])
    for name, want in one["solo"].items():
        if isinstance(want, str):
            assert solo[name] == want
        else:
            assert solo[name].shape == want.shape
    errs.append(_rel(solo["covariance"], one["solo"]["covariance"], np.abs(one["solo"]["covariance"]).max(),
                     f"{what}: covariance on rank 0 alone"))
    assert max(errs) <= TOL, errs


@pytest.mark.parametrize("n_ranks", [2, 3])
@pytest.mark.parametrize("noise", ["scalar", "per_output"])
def test_obs_variance_state_is_within_tol(base, noise, n_ranks):
    """`_corrected_r2` rows, `variance_weights`, the leverage, the leave-one-out residuals and `obs_variance(X)` against
    one rank, at the TOL of everything else (what makes that possible: the module docstring)."""
    one, res = _variance_runs(base, noise, n_ranks)
    what = f"obs_variance {noise}, {n_ranks} ranks"
    errs = [_rel(res[0]["vw"], one["vw"], np.abs(one["vw"]).max(), f"{what}: variance_weights")]
    for key in ("cr2", "h", "loo", "loo_cached"):
        rows = np.concatenate([r[key] for r in res], axis=0)
        errs.append(_rel(rows, one[key], np.abs(one[key]).max(), f"{what}: {key}"))
    for name in ("obs_variance", "get_obs_variance"):
        want = one["solo"][name]
        errs.append(_rel(res[0]["solo"][name], want, np.abs(want).max(), f"{what}: {name} on rank 0 alone"))
    assert max(errs) <= TOL, errs


# ---- 7. one sigma per cell --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ranks", [2, 3])
def test_per_cell_sigma_goes_with_the_cell_shard(base, n_ranks):
    import mellon_amd
    x, y, lm, x_new = base
    y1 = np.ascontiguousarray(y[:, 0])
    sig = 0.2 + 0.3 * np.random.default_rng(23).uniform(size=x.shape[0])
    make = lambda lo, hi: mellon_amd.FunctionEstimator(landmarks=lm, sigma=np.ascontiguousarray(sig[lo:hi]))
    one = _fit_one(x, y1, x_new, make)
    res = _fit_sharded(n_ranks, x, y1, x_new, make)
    assert res[0]["train"].ndim == 1
    _check_against_one_rank(res, one, f"per-cell sigma, {n_ranks} ranks")


# ---- 8. n_obs and JSON -----------------------------------------------------------------------------------------------
def test_n_obs_is_global_and_json_reads_back_in_one_process(base, tmp_path, monkeypatch):
    """The predictor's wire format carries the time of serialisation: with the clock held still the strings of the
    ranks are identical, i.e. everything else in them is."""
    import datetime as dt
    import mellon_amd
    from mellon_amd import base_cov, base_predictor
    x, y, lm, x_new = base

    class Frozen(dt.datetime):
        @classmethod
        def now(cls, tz=None):
            return cls(2024, 1, 1)
    monkeypatch.setattr(base_predictor, "datetime", Frozen)
    monkeypatch.setattr(base_cov, "datetime", Frozen)          # (the covariance's own metadata carries a second stamp)
    make = lambda lo, hi: mellon_amd.FunctionEstimator(landmarks=lm, sigma=SIGMA, predictor_with_uncertainty=True)
    extra = lambda est, comm, lo, hi: dict(json=est.predict.to_json())
    one = _fit_one(x, y, x_new, make, extra)
    res = _fit_sharded(3, x, y, x_new, make, extra)
    assert one["n_obs"] == x.shape[0] and all(r["n_obs"] == x.shape[0] for r in res)
    assert all(r["x_rows"] < x.shape[0] for r in res)
    for r in res[1:]:
        a, b = json.loads(res[0]["json"]), json.loads(r["json"])
        differing = [(part, k) for part in a for k in a[part] if a[part][k] != b[part].get(k)]
        assert r["json"] == res[0]["json"], f"the ranks' JSON differs in {differing}"
    assert json.loads(res[2]["json"])["data"]["n_obs"] == x.shape[0]
    path = tmp_path / "rank2.json"
    path.write_text(res[2]["json"])
    back = mellon_amd.Predictor.from_json(path)
    assert back.n_obs == x.shape[0]
    assert np.array_equal(back(x_new), res[2]["new"])
    assert np.array_equal(back(x[:200]), res[0]["train"][:200])
    assert _rel(back(x_new), one["new"], np.abs(one["new"]).max(), "from_json against one rank") <= TOL


# ---- leverage with shards of different chunk counts ------------------------------------------------------------------
def test_leverage_when_one_shard_spans_two_gram_chunks():
    """mln_kernel_gram all-reduces once per 65536-row chunk, so shards of 70,000 and 1,500 query rows would make
    different numbers of collective calls; conditional._kernel_gram_all_ranks makes none and returns the single-rank
    leverage rows.
    Bound: h_i = b_i^T M^-1 b_i with M = sigma^2 K_uu + S + jitter I, S = B^T B; re-associating the sum S over the rows
    perturbs it by at most gamma |S|, gamma = 64 eps (the partial sums either side forms: at most 16 k-splits x 2 chunks
    x 2 ranks), hence |dh_i| <= h_i |M^-1| gamma |S| <= gamma |S|_2 / lambda_min(M) for h <= 1 (host, NumPy)."""
    import mellon_amd
    from oracle import mellon_oracle as mo
    x, y, lm, _ = make_workload()
    est = mellon_amd.FunctionEstimator(landmarks=lm, sigma=SIGMA)
    est.fit(x, y)
    rng = np.random.default_rng(31)
    q = np.ascontiguousarray(x[rng.integers(0, x.shape[0], size=71_500)] + 0.05 * rng.normal(size=(71_500, x.shape[1])))
    want = est.predict.leverage(q)
    cuts = [0, 70_000, 71_500]

    def body(comm):
        from mellon_amd import distributed
        lo, hi = distributed.shard_bounds(x.shape[0], comm.world_size, comm.rank)
        e = mellon_amd.FunctionEstimator(landmarks=lm, sigma=SIGMA)
        e.fit(np.ascontiguousarray(x[lo:hi]), np.ascontiguousarray(y[lo:hi]))
        return e.predict.leverage(np.ascontiguousarray(q[cuts[comm.rank]:cuts[comm.rank + 1]]))

    got = np.concatenate(_run_ranks(2, body, deadline=120.0))
    cov = mo.compute_cov_func(mo.Matern52, est.ls)
    B = cov(q, lm)
    S = B.T @ B
    M = SIGMA ** 2 * cov(lm, lm) + S + est.jitter * np.eye(lm.shape[0])
    bound = 64 * np.finfo(np.float64).eps * np.linalg.norm(S, 2) / np.linalg.eigvalsh(M)[0]
    err = float(np.abs(got - want).max())
    print(f"leverage over uneven chunks: {err:.3e} (bound {bound:.3e})")
    assert got.shape == want.shape and err <= bound


# ---- 9. two processes on one GPU over the host-staged transport --------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_processes_share_one_gpu(base, one_rank_by_noise, tmp_path):
    port = _free_port()
    world = 2
    procs = []
    # the inputs travel as a file: k-means landmarks computed anew in every process would differ in the last bit
    np.savez(tmp_path / "workload.npz", x=base[0], y=base[1], landmarks=base[2], x_new=base[3])
    for r in range(world):
        env = dict(os.environ)
        env.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), LOCAL_WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), MELLON_AMD_SHARE_GPU="1", MELLON_AMD_COMM_TIMEOUT="120",
                   TORCHELASTIC_RUN_ID=f"fn{port}", PYTHONPATH=ROOT + os.pathsep + env.get("PYTHONPATH", ""))
        procs.append(subprocess.Popen(["timeout", "-k", "10", "300", sys.executable,
                                       os.path.join(ROOT, "tests", "_mp_function_rank_worker.py"), str(tmp_path)],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=400)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    res = [dict(np.load(tmp_path / f"rank{r}.npz")) for r in range(world)]
    assert all(str(r["backend"]) == "host" for r in res)
    assert int(res[0]["lo"]) == 0 and int(res[0]["hi"]) == int(res[1]["lo"]) and int(res[1]["hi"]) == base[0].shape[0]
    assert all(int(r["n_obs"]) == base[0].shape[0] for r in res)
    assert res[0]["new"].shape[0] == N_HELD_OUT
    _check_against_one_rank(res, one_rank_by_noise["scalar"], "two processes")
