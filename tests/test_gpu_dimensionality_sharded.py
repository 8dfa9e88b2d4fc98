"""DimensionalityEstimator with cells sharded over ranks, on ONE MI355X (-m gpu): N thread-ranks joined by the library's
loopback communicator (distributed.run_loopback) run the real sharded path -- every rank searches its own cells among the
cells of all ranks, the loss, both gradient rows and the Hessian diagonal are all-reduced inside mln_dim_objective, SciPy's
L-BFGS-B runs on every rank -- and must reproduce the single-rank estimator and the SciPy solve of the restatement
(tests/dim_restatement.py).  Shards are contiguous, in rank order and deliberately uneven; one case holds a shard with
fewer than k cells.  The last tests run two real processes (host-staged collectives on one GPU; RCCL when there are two)."""
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
from scipy.optimize import minimize

import dim_restatement as dr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cuts_of(n, fractions):
    """Shard boundaries [0, ..., n]: a fraction in (0, 1) is a share of n, an integer a row."""
    inner = [int(round(f * n)) if isinstance(f, float) else int(f) for f in fractions]
    return [0] + inner + [n]


def run_sharded(x, fractions, body):
    """body(comm, lo, hi, x_shard) on len(fractions) + 1 thread-ranks; results in rank order."""
    from mellon_amd import distributed
    cuts = cuts_of(x.shape[0], fractions)

    def rank_body(comm):
        lo, hi = cuts[comm.rank], cuts[comm.rank + 1]
        return body(comm, lo, hi, np.ascontiguousarray(x[lo:hi]))

    return cuts, distributed.run_loopback(len(cuts) - 1, rank_body)


def cells(n, d, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, d)) @ rng.normal(size=(d, d))


# ---- distances and local dimension -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,k,fractions", [
    (1500, 6, 10, (0.37,)),               # k + 1 <= 30: one search of 30 neighbours
    (1500, 6, 40, (0.2, 0.71)),           # 30 < k + 1 <= 64: one search of k + 1
    (700, 4, 64, (0.2, 0.71)),            # k = 64: the self-excluding search (self_offset = lo) and a second one
    (25, 3, 5, (0.37,)),                  # n_global < 30: neighbourhoods of all cells
    (400, 5, 10, (248, 252)),             # the middle shard holds 4 cells < k
])
def test_distances_and_local_dimension_are_rows_of_the_single_rank(n, d, k, fractions):
    import mellon_amd
    x = cells(n, d, seed=n + k)
    one = mellon_amd.DimensionalityEstimator(k=k)
    one.set_x(x)
    for attr in ("distances", "nn_distances", "d"):
        one._prepare_attribute(attr)
    assert one.distances.shape == (n, k) and one.d.shape == (n,)

    def body(comm, lo, hi, xs):
        est = mellon_amd.DimensionalityEstimator(k=k)
        est.set_x(xs)
        est._prepare_attribute("distances")
        idx = est._knn_idx[1].copy()
        for attr in ("nn_distances", "d"):
            est._prepare_attribute(attr)
        return est.distances, est.nn_distances, est.d, idx

    cuts, res = run_sharded(x, fractions, body)
    if fractions == (248, 252):
        assert min(b - a for a, b in zip(cuts[:-1], cuts[1:])) < k
    for r, (dist, nn, dd, idx) in enumerate(res):
        lo, hi = cuts[r], cuts[r + 1]
        assert dist.shape == (hi - lo, k)
        assert np.array_equal(dist, one.distances[lo:hi])          # the same kernel on the same pairs
        assert np.array_equal(nn, one.nn_distances[lo:hi])
        # global indices: column 0 is the cell itself (no coincident cells in this data)
        assert np.array_equal(idx[:, 0], np.arange(lo, hi)) and idx.shape[1] == min(30, n)
        assert idx.min() >= 0 and idx.max() < n
        err = np.abs(dd - one.d[lo:hi])
        print(f"ranks={len(res)} rank={r} rows=[{lo},{hi}) max |d - d_single| = {err.max():.3e}")
        assert np.all(err <= 1e-12 * np.maximum(1.0, np.abs(one.d[lo:hi])))
    want = dr.local_dimensionality(x)
    np.testing.assert_allclose(np.concatenate([r[2] for r in res]), want, rtol=1e-10)


# ---- objective -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fractions", [(0.37,), (0.2, 0.71)])
def test_objective_on_shards_equals_single_rank(fractions):
    import mellon_amd
    n, d, m = 1800, 5, 120
    x = cells(n, d, seed=3)
    one = mellon_amd.DimensionalityEstimator(n_landmarks=m, predictor_with_uncertainty=True)
    loss_func, z0 = one.prepare_inference(x)
    rng = np.random.default_rng(8)
    z = z0 + 0.05 * rng.normal(size=z0.shape)
    u = loss_func.u_from_z(z)
    want = dict(vg=loss_func.value_and_grad(z), vgu=loss_func.value_and_grad_u(u), h=loss_func.hessian_diagonal(z))
    # ... and the single rank itself is the restatement's objective (the suite's gates for it)
    L, ell = np.asarray(one.L), dr.ell_of(one.distances)
    ref_loss = dr.dim_loss(z, L, ell, one.mu_dim, one.mu_dens)
    ref_g, ref_h = dr.dim_grad_hess(z, L, ell, one.mu_dim, one.mu_dens)
    landmarks = np.ascontiguousarray(one.landmarks)

    def body(comm, lo, hi, xs):
        est = mellon_amd.DimensionalityEstimator(landmarks=landmarks, predictor_with_uncertainty=True)
        lf, start = est.prepare_inference(xs)
        return dict(vg=lf.value_and_grad(z), vgu=lf.value_and_grad_u(u), h=lf.hessian_diagonal(z), start=start,
                    mu_dens=est.mu_dens, ls=est.ls)

    cuts, res = run_sharded(x, fractions, body)
    for r in res:
        for key in ("vg", "vgu"):
            loss, g = r[key]
            wl, wg = want[key]
            print(f"ranks={len(res)} {key}: |loss - single| / |single| = {abs(loss - wl) / abs(wl):.3e}, "
                  f"max |g - single| / max |single| = {np.abs(g - wg).max() / np.abs(wg).max():.3e}")
            assert abs(loss - wl) <= 1e-11 * abs(wl)
            assert np.abs(g - wg).max() <= 1e-9 * np.abs(wg).max()
        print(f"ranks={len(res)} hessian diagonal: {np.abs(r['h'] - want['h']).max() / np.abs(want['h']).max():.3e}")
        assert np.abs(r["h"] - want["h"]).max() <= 1e-9 * np.abs(want["h"]).max()
        assert abs(r["vg"][0] - ref_loss) <= 1e-11 * abs(ref_loss)
        assert np.abs(r["vg"][1] - ref_g).max() <= 1e-9 * np.abs(ref_g).max()
        assert np.abs(r["h"] - ref_h).max() <= 1e-9 * np.abs(ref_h).max()
        # the start (exact Ridge over the cells of all ranks) is the single rank's
        np.testing.assert_allclose(r["start"], z0, rtol=1e-8, atol=1e-10)
        assert abs(r["mu_dens"] - one.mu_dens) <= 1e-12 * abs(one.mu_dens) and abs(r["ls"] / one.ls - 1) <= 1e-12
    # every rank holds the same bits: one optimiser path, the same number of collective calls
    for r in res[1:]:
        for key in ("vg", "vgu"):
            assert r[key][0] == res[0][key][0] and np.array_equal(r[key][1], res[0][key][1])
        assert np.array_equal(r["h"], res[0]["h"]) and np.array_equal(r["start"], res[0]["start"])
        assert r["mu_dens"] == res[0]["mu_dens"] and r["ls"] == res[0]["ls"]


# ---- full fit ----------------------------------------------------------------------------------------------------------
def expected_from_restatement(L, distances, d, nn, mu_dim, mu_dens):
    """The reference's initial value and a SciPy solve of the restatement from it, exactly as
    test_gpu_dimensionality.py::test_estimator_end_to_end_matches_scipy_solve_of_restatement builds them."""
    ell = dr.ell_of(distances)
    z0 = dr.initial_dimensionalities(L, d, mu_dim, nn, mu_dens)
    res = minimize(lambda z: (dr.dim_loss(z, L, ell, mu_dim, mu_dens),
                              dr.dim_grad_hess(z, L, ell, mu_dim, mu_dens)[0].ravel()),
                   z0.ravel(), jac=True, method="L-BFGS-B", options=dict(maxiter=20000, maxfun=50000, ftol=1e-15, gtol=1e-9))
    z = res.x.reshape(2, -1)
    return z0, np.exp(mu_dim + L @ z[0]), mu_dens + L @ z[1]


@pytest.mark.parametrize("fractions", [(0.37,), (0.2, 0.71)])
def test_sharded_fit_matches_scipy_solve_of_restatement(fractions):
    """Raises NotImplementedError without the sharded estimator layer."""
    import mellon_amd
    rng = np.random.default_rng(21)
    x = rng.normal(size=(2000, 5))
    x_new = x[::7] + 0.01

    def body(comm, lo, hi, xs):
        est = mellon_amd.DimensionalityEstimator(n_landmarks=200, predictor_with_uncertainty=True)
        dim = est.fit_predict(xs)
        return dict(dim=dim, dens=est.log_density_x, z=est.pre_transformation, std=est.pre_transformation_std,
                    L=np.asarray(est.L), distances=est.distances, d=est.d, nn=est.nn_distances, mu_dim=est.mu_dim,
                    mu_dens=est.mu_dens, start=est.initial_value, loss=est.losses[-1], n_eval=est.loss_func.n_eval,
                    landmarks=np.asarray(est.landmarks), pred=est.predict(x), pred_dens=est.predict_density(x),
                    pred_new=est.predict(x_new), unc=est.predict.uncertainty(x_new))

    cuts, res = run_sharded(x, fractions, body)
    for r, (lo, hi) in zip(res, zip(cuts[:-1], cuts[1:])):
        assert r["dim"].shape == (hi - lo,) and r["dens"].shape == (hi - lo,) and r["L"].shape[0] == hi - lo
    first = res[0]
    m = first["L"].shape[1]
    for r in res:
        assert np.array_equal(r["z"], first["z"]) and r["z"].shape == (2, m)     # one optimiser path on every rank
        assert r["std"].shape == (2, m) and np.array_equal(r["std"], first["std"])
        assert r["loss"] == first["loss"] and r["n_eval"] == first["n_eval"]
        assert np.array_equal(r["landmarks"], first["landmarks"]) and r["mu_dens"] == first["mu_dens"]
        for key in ("pred", "pred_dens", "pred_new", "unc"):                       # predictors: replicated state only
            assert np.array_equal(r[key], first[key]), key
    L = np.concatenate([r["L"] for r in res])
    distances = np.concatenate([r["distances"] for r in res])
    d = np.concatenate([r["d"] for r in res])
    nn = np.concatenate([r["nn"] for r in res])
    dim = np.concatenate([r["dim"] for r in res])
    dens = np.concatenate([r["dens"] for r in res])
    mu_dim, mu_dens = first["mu_dim"], first["mu_dens"]
    ell = dr.ell_of(distances)
    loss = dr.dim_loss(first["z"], L, ell, mu_dim, mu_dens)
    g, _ = dr.dim_grad_hess(first["z"], L, ell, mu_dim, mu_dens)
    assert np.abs(g).max() <= 1e-5 * max(1.0, abs(loss))
    assert abs(first["loss"] - loss) <= 1e-9 * abs(loss)
    np.testing.assert_allclose(d, dr.local_dimensionality(x), rtol=1e-10)
    z0, want_dim, want_dens = expected_from_restatement(L, distances, d, nn, mu_dim, mu_dens)
    np.testing.assert_allclose(first["start"], z0, rtol=1e-8, atol=1e-10)
    e_dim = np.abs(dim - want_dim).max() / np.abs(want_dim).max()
    e_dens = np.abs(dens - want_dens).max() / np.abs(want_dens).max()
    print(f"ranks={len(res)} evaluations={first['n_eval']} local_dim_x: {e_dim:.3e} log_density_x: {e_dens:.3e} (gate 1e-5)")
    assert e_dim <= 1e-5
    assert e_dens <= 1e-5
    # the replicated predictor reproduces the fitted rows of all ranks
    assert np.abs(first["pred"] - dim).max() <= 1e-4 * np.abs(dim).max()
    assert np.all(np.isfinite(first["unc"])) and first["unc"].shape == (x_new.shape[0],)


def test_sharded_fit_with_a_shard_smaller_than_k():
    """A shard of 4 cells (k = 10) fits: k, gp_type and n_landmarks are decided on the global count."""
    import mellon_amd
    x = cells(600, 4, seed=5)
    one = mellon_amd.DimensionalityEstimator(n_landmarks=60)
    dim1 = one.fit_predict(x)

    def body(comm, lo, hi, xs):
        est = mellon_amd.DimensionalityEstimator(n_landmarks=60)
        dim = est.fit_predict(xs)
        return dim, est.log_density_x, str(est.gp_type), est.n_landmarks, est.pre_transformation

    cuts, res = run_sharded(x, (298, 302), body)
    assert [r[0].shape[0] for r in res] == [298, 4, 298]
    assert all(r[2] == str(one.gp_type) and r[3] == 60 and np.array_equal(r[4], res[0][4]) for r in res)
    # both fits pass the suite's 1e-5 gate against the same optimum; against each other that leaves 2e-5
    dim = np.concatenate([r[0] for r in res])
    dens = np.concatenate([r[1] for r in res])
    assert np.abs(dim - dim1).max() <= 2e-5 * np.abs(dim1).max()
    assert np.abs(dens - one.log_density_x).max() <= 2e-5 * np.abs(one.log_density_x).max()


# ---- errors ------------------------------------------------------------------------------------------------------------
def test_duplicates_across_ranks_raise_on_every_rank():
    """Three cells of rank 0 repeated on the last rank: 6 cells have a zero nearest-neighbour distance, none of the
    pairs lies within one rank.  Every rank raises the same ValueError; nobody is left waiting in a collective."""
    import mellon_amd
    from mellon_amd import distributed
    x = cells(900, 4, seed=12)
    x[-3:] = x[:3]

    def body(comm, lo, hi, xs):
        try:
            mellon_amd.DimensionalityEstimator(n_landmarks=50).fit(xs)
        except ValueError as e:
            return str(e)
        return None

    for fractions in ((0.37,), (0.2, 0.71)):
        _, res = run_sharded(x, fractions, body)
        assert all(r is not None and r.startswith("6 cells have a nearest-neighbour distance of 0") for r in res), res
        assert len(set(res)) == 1

    def raising(comm, lo, hi, xs):
        mellon_amd.DimensionalityEstimator(n_landmarks=50).fit(xs)

    with pytest.raises(ValueError, match="6 cells"):        # ... and run_loopback returns instead of hanging
        run_sharded(x, (0.2, 0.71), raising)

    # the local-dimension check (user-given distances skip the first one): the count is the global one too
    def dim_check(comm, lo, hi, xs):
        est = mellon_amd.DimensionalityEstimator(n_landmarks=50, distances=np.ones((hi - lo, 10)))
        try:
            est.fit(xs)
        except ValueError as e:
            return str(e)
        return None

    _, res = run_sharded(x, (0.2, 0.71), dim_check)
    single = mellon_amd.DimensionalityEstimator(n_landmarks=50, distances=np.ones((x.shape[0], 10)))
    with pytest.raises(ValueError, match="non-finite local dimension") as info:
        single.fit(x)
    assert all(r == str(info.value) for r in res), (res, str(info.value))
    assert distributed.current().world_size == 1


def test_k_is_validated_against_the_global_count():
    import mellon_amd
    x = cells(40, 3, seed=1)

    def body(comm, lo, hi, xs):
        out = []
        for k in (40, 39):          # k must be smaller than the 40 cells of all ranks; 39 is legal though no shard holds 39
            est = mellon_amd.DimensionalityEstimator(k=k)
            est.set_x(xs)
            try:
                est._prepare_attribute("distances")
                out.append(est.distances.shape)
            except ValueError as e:
                out.append(str(e))
        return out

    _, res = run_sharded(x, (0.2, 0.71), body)
    for r, rows in zip(res, (8, 20, 12)):
        assert r[0] == "k=40 must be smaller than the number of samples 40."
        assert r[1] == (rows, 39)


# ---- d_method="fractal" ------------------------------------------------------------------------------------------------
def test_fractal_d_under_ranks():
    import mellon_amd
    rng = np.random.default_rng(2)
    x = rng.normal(size=(1200, 3)) @ rng.normal(size=(3, 5))          # more than 500 cells: the draw matters
    one = mellon_amd.DensityEstimator(d_method="fractal", n_landmarks=50)
    one.prepare_inference(x)
    assert abs(one.d - dr.fractal_d(x)) <= 1e-10 * abs(one.d)
    xt = np.concatenate([x, np.repeat([0.0, 1.0, 2.0], 400)[:, None]], axis=1)

    def body(comm, lo, hi, xs):
        est = mellon_amd.DensityEstimator(d_method="fractal", n_landmarks=50)
        est.prepare_inference(xs)
        ts = mellon_amd.TimeSensitiveDensityEstimator(d_method="fractal", n_landmarks=50, ls_time=1.0)
        ts.set_x(np.ascontiguousarray(xt[lo:hi]))
        ts._prepare_attribute("d")
        return est.d, ts.d

    _, res = run_sharded(x, (0.37,), body)
    assert all(r[0] == one.d and r[1] == one.d for r in res), (res, one.d)


# ---- two real processes ------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _launch_ranks(tmp_path, world, share_gpu, limit=420):
    """Start `world` fresh worker processes, each under a time limit of its own; stop at the first non-zero exit."""
    port = _free_port()
    procs = []
    for rank in range(world):
        env = dict(os.environ)
        env.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), LOCAL_WORLD_SIZE=str(world),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), MELLON_AMD_COMM_TIMEOUT="120",
                   TORCHELASTIC_RUN_ID=f"dim{port}", PYTHONPATH=ROOT + os.pathsep + env.get("PYTHONPATH", ""))
        if share_gpu:
            env["MELLON_AMD_SHARE_GPU"] = "1"
        else:
            env.pop("MELLON_AMD_SHARE_GPU", None)
            env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
        log = open(tmp_path / f"rank{rank}.log", "w")
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.join(ROOT, "tests", "_mp_dim_rank_worker.py"),
               str(tmp_path)]
        procs.append((subprocess.Popen(cmd, env=env, stdout=log, stderr=subprocess.STDOUT), log))
    failed = None
    try:
        pending = list(range(world))
        while pending and failed is None:
            time.sleep(0.2)
            for rank in list(pending):
                code = procs[rank][0].poll()
                if code is None:
                    continue
                pending.remove(rank)
                if code != 0:
                    failed = (rank, code)
                    break
    finally:
        for p, log in procs:
            if p.poll() is None:
                p.kill()
            p.wait()
            log.close()
    logs = "\n".join(f"--- rank {r} ---\n" + open(tmp_path / f"rank{r}.log").read()[-3000:] for r in range(world))
    assert failed is None, f"rank {failed[0]} exited with {failed[1]}\n{logs}"
    return [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]


def _check_process_results(res, backend):
    import mellon_amd
    n, d = 3000, 5
    x = np.random.default_rng(33).normal(size=(n, d))
    assert all(str(r["backend"]) == backend and bool(r["self_test_ok"]) for r in res)
    assert int(res[0]["lo"]) == 0 and int(res[-1]["hi"]) == n
    assert all(int(a["hi"]) == int(b["lo"]) for a, b in zip(res[:-1], res[1:]))
    assert int(res[0]["hi"]) == 1110                                  # the uneven cut the worker makes
    for r in res[1:]:
        for key in ("z", "std", "landmarks", "pred", "pred_dens"):
            assert np.array_equal(r[key], res[0][key]), key
        assert float(r["mu_dens"]) == float(res[0]["mu_dens"]) and int(r["n_eval"]) == int(res[0]["n_eval"])
    one = mellon_amd.DimensionalityEstimator(k=10)
    one.set_x(x)
    one._prepare_attribute("distances")
    distances = np.concatenate([r["distances"] for r in res])
    assert np.array_equal(distances, one.distances)
    L = np.concatenate([r["L"] for r in res])
    dd = np.concatenate([r["d"] for r in res])
    nn = np.concatenate([r["nn"] for r in res])
    _, want_dim, want_dens = expected_from_restatement(L, distances, dd, nn, float(res[0]["mu_dim"]),
                                                       float(res[0]["mu_dens"]))
    dim = np.concatenate([r["dim"] for r in res])
    dens = np.concatenate([r["dens"] for r in res])
    e_dim = np.abs(dim - want_dim).max() / np.abs(want_dim).max()
    e_dens = np.abs(dens - want_dens).max() / np.abs(want_dens).max()
    print(f"processes={len(res)} backend={backend} local_dim_x: {e_dim:.3e} log_density_x: {e_dens:.3e} (gate 1e-5)")
    assert e_dim <= 1e-5 and e_dens <= 1e-5
    assert res[0]["std"].shape == (2, L.shape[1])


def test_two_processes_on_one_gpu(tmp_path):
    """Two processes under the launcher's environment variables share GPU 0; the device collectives of
    mln_dim_objective, the Ridge Gram and the factorisation travel host-staged (mln_comm_init_host)."""
    _check_process_results(_launch_ranks(tmp_path, 2, share_gpu=True), "host")


def test_two_processes_over_rccl_when_there_are_two_devices(tmp_path):
    from mellon_amd import _lib
    if _lib.device_count() < 2:
        pytest.skip("one visible device: RCCL with two ranks needs two")
    _check_process_results(_launch_ranks(tmp_path, 2, share_gpu=False), "rccl")
