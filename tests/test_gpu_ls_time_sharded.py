"""The automatic `ls_time` of TimeSensitiveDensityEstimator on cell-sharded input (-m gpu): N thread-ranks on one GPU
(distributed.run_loopback) and one two-process run over the host-staged transport.

Data: d = 5 state columns, T = 3 time points of 1500, 1200 and 900 cells -- one Gaussian mixture, shifted by 0.4 per time
unit in every column -- with the rows sorted by time.  Three contiguous shards of 1200 rows then leave rank 0 with time
point 0 only and rank 2 without a cell of it (300 cells of time point 1, all of time point 2): the case the per-time-point
re-sharding exists for."""
import functools
import os
import socket
import subprocess
import sys
import threading

import numpy as np
import pytest

from oracle import mellon_oracle as mo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES, DIMS, SHIFT, N_LANDMARKS = (1500, 1200, 900), 5, 0.4, 100

# Relative margin between the sharded and the single-rank ls_time.  Fixed from the single-rank path alone: its T x n
# table (this data, mixture seeds 21..25) perturbed entry-wise by a relative 1e-6 -- the gate the nested sharded fits are
# held to, random signs, 8 draws per seed -- and ls_time recomputed with the unchanged single-rank code
# (_correlation_of_rows + _closest_length_scale).  Largest relative change measured: LS_TIME_SENSITIVITY; the factor 4
# covers the noise of the finite-difference L-BFGS-B search itself.
LS_TIME_SENSITIVITY = 4.999502e-07        # measured on the MI355X (per seed: 3.4e-7, 4.5e-7, 5.0e-7, 4.5e-7, 3.2e-7)
LS_TIME_TOL = 4 * LS_TIME_SENSITIVITY


def time_series(seed=21):
    """(x [n x 5], times [n]) of the module docstring."""
    x = mo.gaussian_mixture(sum(SIZES), DIMS, seed=seed)
    times = np.repeat(np.arange(float(len(SIZES))), SIZES)
    return np.ascontiguousarray(x + SHIFT * times[:, None]), times


def probe_cells(x):
    return np.ascontiguousarray(x[::57][:64])


def _nested(nested_landmarks):
    return {} if nested_landmarks is None else dict(density_estimator_kwargs=dict(n_landmarks=nested_landmarks))


@functools.lru_cache(maxsize=None)
def _single(nested_landmarks=None):
    """The single-rank default fit with its intermediates, computed once."""
    import mellon_amd
    x, times = time_series()
    est = mellon_amd.TimeSensitiveDensityEstimator(n_landmarks=N_LANDMARKS, _save_intermediate_ls_times=True,
                                                   **_nested(nested_landmarks))
    est.fit(x, times)
    probes = [np.asarray(model.predict(probe_cells(x))) for model in est.predictors]
    return dict(ls_time=est.ls_time, stages=np.asarray(est.numeric_stages), probes=probes)


@functools.lru_cache(maxsize=None)
def _single_given(ls_time):
    import mellon_amd
    x, times = time_series()
    est = mellon_amd.TimeSensitiveDensityEstimator(n_landmarks=N_LANDMARKS, ls_time=ls_time)
    return np.asarray(est.fit_predict(x, times))


@functools.lru_cache(maxsize=None)
def _sharded(n_ranks, save=False, nested_landmarks=None):
    import mellon_amd
    from mellon_amd import distributed
    x, times = time_series()
    probe = probe_cells(x)

    def body(comm):
        lo, hi = distributed.shard_bounds(x.shape[0], comm.world_size, comm.rank)
        est = mellon_amd.TimeSensitiveDensityEstimator(n_landmarks=N_LANDMARKS, _save_intermediate_ls_times=save,
                                                       **_nested(nested_landmarks))
        est.fit(np.ascontiguousarray(x[lo:hi]), np.ascontiguousarray(times[lo:hi]))
        out = dict(ls_time=est.ls_time, cov_func=str(est.cov_func), landmarks=np.array(est.landmarks),
                   z=np.array(est.pre_transformation), dens=np.array(est.log_density_x), lo=lo, hi=hi,
                   stamps=sorted(set(times[lo:hi])))
        if save:
            out.update(stages=np.asarray(est.numeric_stages), densities=np.asarray(est.densities),
                       probes=[np.asarray(model.predict(probe)) for model in est.predictors],
                       local=[np.asarray(model.predict(x[lo:hi])) for model in est.predictors])
        return out

    return distributed.run_loopback(n_ranks, body)


@pytest.mark.parametrize("n_ranks", [2, 3, 4])
def test_default_call_on_sharded_cells(n_ranks):
    """TimeSensitiveDensityEstimator(n_landmarks=100).fit(x_shard, times_shard) with no ls_time returns on every rank, with
    one ls_time and one model everywhere, and the density of a single-rank fit that is handed that ls_time."""
    res = _sharded(n_ranks)
    if n_ranks == 3:
        assert res[0]["stamps"] == [0.0] and res[2]["stamps"] == [1.0, 2.0]     # the shards miss whole time points
    assert all(r["ls_time"] == res[0]["ls_time"] for r in res), [r["ls_time"] for r in res]
    assert res[0]["ls_time"] > 0 and np.isfinite(res[0]["ls_time"])
    assert all(r["cov_func"] == res[0]["cov_func"] for r in res)
    assert all(np.array_equal(r["landmarks"], res[0]["landmarks"]) for r in res)
    assert all(np.array_equal(r["z"], res[0]["z"]) for r in res)
    dens = np.concatenate([r["dens"] for r in res])
    one = _single_given(res[0]["ls_time"])
    err = np.abs(dens - one).max() / np.abs(one).max()
    print(f"ranks={n_ranks} ls_time={res[0]['ls_time']!r} density vs single rank: {err:.3e}")
    assert dens.shape == one.shape and err < 1e-6, err


def test_per_time_point_predictors_match_the_single_rank_ones():
    """_save_intermediate_ls_times under 3 ranks: the global stamps, replicated predictors that agree with the single-rank
    run's on 64 probe cells, and this rank's T x n_local columns of the table."""
    one, res = _single(), _sharded(3, save=True)
    for r in res:
        assert np.array_equal(r["stages"], one["stages"]) and r["stages"].dtype == one["stages"].dtype
        assert r["densities"].shape == (len(SIZES), r["hi"] - r["lo"])
        for t in range(len(SIZES)):
            assert np.array_equal(r["probes"][t], res[0]["probes"][t])            # replicated: the same bits
            scale = np.abs(one["probes"][t]).max()
            err = np.abs(r["probes"][t] - one["probes"][t]).max() / scale
            print(f"rank {r['lo']}..{r['hi']} time point {t}: predictor vs single rank {err:.3e}")
            assert err < 1e-6, (t, err)
            # the table in HBM holds what the predictor returns to the host (the same fused pass)
            assert np.abs(r["densities"][t] - r["local"][t]).max() <= 1e-12 * scale


def test_sparse_nested_fits_decide_on_the_global_cell_count():
    """density_estimator_kwargs=dict(n_landmarks=400): the nested fits are sparse (k-means landmarks from the gathered
    cells, the library's own cell-sharded factorisation).  Under 3 ranks the slices hold 500, 400 and 300 cells: a decision
    on the local count would call the second time point non-sparse and refuse the third; decided on n_t they are what one
    rank fits.  Same gates: predictors to 1e-6 of scale, ls_time within the single-rank path's own sensitivity (the table
    approximates the same three densities)."""
    one, res = _single(400), _sharded(3, save=True, nested_landmarks=400)
    assert all(r["ls_time"] == res[0]["ls_time"] for r in res)
    for t in range(len(SIZES)):
        assert all(np.array_equal(r["probes"][t], res[0]["probes"][t]) for r in res)
        err = np.abs(res[0]["probes"][t] - one["probes"][t]).max() / np.abs(one["probes"][t]).max()
        print(f"sparse nested fit, time point {t}: predictor vs single rank {err:.3e}")
        assert err < 1e-6, (t, err)
    rel = abs(res[0]["ls_time"] - one["ls_time"]) / one["ls_time"]
    print(f"sparse nested fits: ls_time sharded {res[0]['ls_time']!r} single {one['ls_time']!r} relative difference {rel:.3e}")
    assert rel <= LS_TIME_TOL, (rel, LS_TIME_TOL)


@pytest.mark.parametrize("n_ranks", [2, 3, 4])
def test_ls_time_equals_the_single_rank_value_within_its_own_sensitivity(n_ranks):
    ls_single, ls_sharded = _single()["ls_time"], _sharded(n_ranks)[0]["ls_time"]
    rel = abs(ls_sharded - ls_single) / ls_single
    print(f"ranks={n_ranks} ls_time sharded {ls_sharded!r} single {ls_single!r} relative difference {rel:.3e} "
          f"(tol {LS_TIME_TOL:.3e})")
    assert abs(ls_sharded - ls_single) <= LS_TIME_TOL * ls_single, (rel, LS_TIME_TOL)
    saved = _sharded(3, save=True)[0]["ls_time"]
    assert n_ranks != 3 or saved == ls_sharded          # storing the intermediates does not change the value


def test_time_point_with_fewer_cells_than_ranks_raises_everywhere():
    """4 ranks, a time point of 3 cells: every rank raises the same ValueError naming the time point and both counts
    (decided on global counts before the nested fit starts, so nobody is left waiting in a collective)."""
    import mellon_amd
    from mellon_amd import distributed
    x = mo.gaussian_mixture(1603, DIMS, seed=31)
    times = np.repeat([0.0, 1.0, 2.0], [800, 3, 800])
    box = {}

    def body(comm):
        lo, hi = distributed.shard_bounds(x.shape[0], comm.world_size, comm.rank)
        est = mellon_amd.TimeSensitiveDensityEstimator(n_landmarks=N_LANDMARKS)
        try:
            est.fit(np.ascontiguousarray(x[lo:hi]), np.ascontiguousarray(times[lo:hi]))
        except ValueError as e:
            return str(e)
        return None

    def run():
        try:
            box["res"] = distributed.run_loopback(4, body)
        except BaseException as e:      # noqa: BLE001 -- reported below
            box["error"] = e

    t = threading.Thread(target=run, daemon=True)
    t.start()
    t.join(120)
    assert not t.is_alive(), "the ranks hang"
    assert "error" not in box, box.get("error")
    msgs = box["res"]
    assert all(m is not None and m == msgs[0] for m in msgs), msgs
    assert "Time point 1.0 has 3 cells but the fit runs on 4 ranks" in msgs[0]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_default_call_in_two_processes(tmp_path):
    """The same fit as two PROCESSES sharing GPU 0, device collectives staged through host memory."""
    port, world = _free_port(), 2
    procs = []
    for r in range(world):
        env = dict(os.environ)
        env.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), LOCAL_WORLD_SIZE=str(world),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), MELLON_AMD_SHARE_GPU="1",
                   MELLON_AMD_COMM_TIMEOUT="120", TORCHELASTIC_RUN_ID=f"lst{port}",
                   PYTHONPATH=ROOT + os.pathsep + env.get("PYTHONPATH", ""))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_mp_ls_time_rank_worker.py"),
                                       str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                      text=True))
    try:
        for r, p in enumerate(procs):          # each child under its own limit; the first failure ends the test
            out = p.communicate(timeout=240)[0]
            assert p.returncode == 0, f"rank {r} exited with {p.returncode}\n{out[-4000:]}"
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
    res = [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]
    assert all(str(r["backend"]) == "host" for r in res)
    ls_time = float(res[0]["ls_time"])
    assert all(float(r["ls_time"]) == ls_time for r in res)
    assert all(np.array_equal(r["landmarks"], res[0]["landmarks"]) and np.array_equal(r["z"], res[0]["z"]) for r in res)
    dens = np.concatenate([r["dens"] for r in res])
    one = _single_given(ls_time)
    err = np.abs(dens - one).max() / np.abs(one).max()
    rel = abs(ls_time - _single()["ls_time"]) / _single()["ls_time"]
    print(f"two processes: ls_time={ls_time!r} density vs single rank {err:.3e}, ls_time vs single rank {rel:.3e}")
    assert err < 1e-6, err
    assert rel <= LS_TIME_TOL, (rel, LS_TIME_TOL)
