"""CPU tests of the host-side mirror (no GPU, no compute calls through the C-ABI):
validators, decision tables, active-dims composition, heuristics, wire formats."""
import json
import os

import numpy as np
import pytest

from oracle import mellon_oracle as mo


def test_gp_type_rank_landmark_tables():
    # reference tests/test_parameters.py:271-365
    from mellon_amd.parameters import compute_gp_type, compute_n_landmarks, compute_rank
    from mellon_amd.util import GaussianProcessType as G
    assert compute_gp_type(0, 100, 100) == G.FULL
    assert compute_gp_type(100, 1.0, 100) == G.FULL
    assert compute_gp_type(100, None, 100) == G.FULL
    assert compute_gp_type(100, 0, 100) == G.FULL
    assert compute_gp_type(100, 50, 100) == G.FULL_NYSTROEM
    assert compute_gp_type(100, 0.5, 100) == G.FULL_NYSTROEM
    assert compute_gp_type(50, 50, 100) == G.SPARSE_CHOLESKY
    assert compute_gp_type(50, 1.0, 100) == G.SPARSE_CHOLESKY
    assert compute_gp_type(50, None, 100) == G.SPARSE_CHOLESKY
    assert compute_gp_type(50, 0, 100) == G.SPARSE_CHOLESKY
    assert compute_gp_type(50, 25, 100) == G.SPARSE_NYSTROEM
    assert compute_gp_type(50, 0.5, 100) == G.SPARSE_NYSTROEM
    assert compute_rank(G.FULL_NYSTROEM) == 0.99 and compute_rank(G.SPARSE_CHOLESKY) == 1.0 and compute_rank(None) == 1.0
    assert compute_n_landmarks(None, 100, np.ones((50, 2))) == 50
    assert compute_n_landmarks(None, 100, None) == 100
    assert compute_n_landmarks(G.FULL, 100, None) == 100
    assert compute_n_landmarks(G.FULL_NYSTROEM, 100, None) == 100
    assert compute_n_landmarks(G.SPARSE_CHOLESKY, 100, None) == 5000
    assert compute_n_landmarks(G.SPARSE_NYSTROEM, 80, None) == 5000
    assert G.from_string("sparse_cholesky") == G.SPARSE_CHOLESKY and G.from_string(None, optional=True) is None
    assert G.FULL == "full"                      # str-enum: literals interchangeable (util.py:589-667)
    with pytest.raises(ValueError):
        G.from_string("no-such-type")


def test_heuristics_match_oracle():
    from mellon_amd import parameters as P
    from mellon_amd.inference import nn_likelihood_constants
    from mellon_amd.util import mle
    rng = np.random.default_rng(0)
    nn = rng.uniform(0.05, 2.0, size=1000)
    assert P.compute_mu(nn, 7) == mo.compute_mu(nn, 7)
    assert P.compute_ls(nn) == pytest.approx(mo.compute_ls(nn), rel=1e-15)
    assert np.array_equal(mle(nn, 7), mo.mle(nn, 7))
    V, Vdr = nn_likelihood_constants(nn, 7)
    Vo, Vdro = mo.nn_likelihood_constants(nn, 7)
    assert np.array_equal(V, Vo) and np.array_equal(Vdr, Vdro)
    dv = rng.uniform(2, 9, size=1000)             # per-cell d (validation allows iterables)
    V, Vdr = nn_likelihood_constants(nn, dv)
    Vo, Vdro = mo.nn_likelihood_constants(nn, dv)
    assert np.allclose(V, Vo) and np.allclose(Vdr, Vdro)
    c = P.compute_cov_func(__import__("mellon_amd").cov.Matern52, 1.5, ls_time=0.3)
    # attribute order follows the reference's __dict__ order (base ctor sets active_dims first)
    assert repr(c) == "(Matern52(active_dims=slice(None, -1, None), ls=1.5) * Matern52(active_dims=-1, ls=0.3))"
    assert repr(__import__("mellon_amd").cov.Matern52(2.0)) == "Matern52(ls=2.0)"


def test_validators():
    from mellon_amd import validation as V
    with pytest.raises(TypeError):
        V.validate_array(None, "x")
    assert V.validate_array(None, "x", optional=True) is None
    with pytest.raises(TypeError):
        V.validate_array(object(), "x")
    a = V.validate_array([[1, 2], [3, 4]], "x")
    assert a.dtype == np.float64 and a.shape == (2, 2)
    with pytest.raises(ValueError):
        V.validate_array(np.zeros((2, 2, 2)), "x", ndim=2)
    with pytest.raises(ValueError):
        V.validate_positive_int(-1, "n")
    assert V.validate_positive_int(0, "n") == 0 and V.validate_positive_int(None, "n", optional=True) is None
    with pytest.raises(ValueError):
        V.validate_positive_float(-0.1, "j")
    with pytest.raises(ValueError):
        V.validate_float(float("nan"), "mu")
    with pytest.raises(TypeError):
        V.validate_bool(1, "flag")
    with pytest.raises(ValueError):
        V.validate_string("sgd", "optimizer", choices={"adam", "advi", "L-BFGS-B"})
    # validation.py:528-592: invalid distances are replaced by the smallest positive one
    nn = V.validate_nn_distances(np.array([0.5, 0.0, np.nan, np.inf, -1.0, 0.2]))
    assert np.array_equal(nn, np.array([0.5, 0.2, 0.2, 0.2, 0.2, 0.2]))
    with pytest.raises(ValueError):
        V.validate_nn_distances(np.array([0.0, np.nan]))
    # validation.py:23-102
    x = np.arange(6.0).reshape(3, 2)
    xt = V.validate_time_x(x, np.array([0.0, 1.0, 2.0]))
    assert xt.shape == (3, 3) and np.array_equal(xt[:, -1], [0, 1, 2])
    assert np.array_equal(V.validate_time_x(x, 5.0, cast_scalar=True)[:, -1], [5, 5, 5])
    with pytest.raises(ValueError):
        V.validate_time_x(x, np.zeros(4))
    with pytest.raises(ValueError):
        V.validate_time_x(x, None, n_features=3)


def test_parameter_validation():
    from mellon_amd.parameter_validation import validate_params
    from mellon_amd.util import GaussianProcessType as G
    validate_params(1.0, G.SPARSE_CHOLESKY, 100, 10, None)
    validate_params(1.0, G.FULL, 100, 100, None)
    with pytest.raises(ValueError):
        validate_params(1.0, G.SPARSE_CHOLESKY, 100, 0, None)
    with pytest.raises(ValueError):
        validate_params(1.0, G.FULL, 100, 10, None)
    with pytest.raises(ValueError):
        validate_params(0.5, G.SPARSE_CHOLESKY, 100, 10, None)       # rank indicates Nystroem
    with pytest.raises(ValueError):
        validate_params(1.0, G.SPARSE_CHOLESKY, 100, 10, np.ones((5, 2)))
    with pytest.raises(ValueError):
        validate_params(1.0, "full", 100, 100, None)


def test_estimator_constructor_validation():
    import mellon_amd as m
    with pytest.raises(ValueError):
        m.DensityEstimator(jitter=-1.0)
    with pytest.raises(ValueError):
        m.DensityEstimator(optimizer="sgd")
    with pytest.raises(ValueError):
        m.DensityEstimator(cov_func="matern")
    with pytest.raises(ValueError):
        m.FunctionEstimator(gp_type="sparse_nystroem")
    est = m.DensityEstimator(d=3.0)
    assert est.d_method == "manual"
    with pytest.raises(ValueError):
        est.fit_predict()                              # no x
    with pytest.raises(ValueError):
        m.TimeSensitiveDensityEstimator(ls_time=-1.0)


def test_predictor_wire_format_without_gpu():
    """State dict layout of base_predictor.py:541-590 and round trip (no device call involved)."""
    import mellon_amd as m
    from mellon_amd.conditional import LandmarksConditionalCholesky
    p = LandmarksConditionalCholesky.__new__(LandmarksConditionalCholesky)
    m.Predictor.__init__(p, m.cov.Matern52(1.2), np.arange(6.0).reshape(3, 2), np.array([0.1, 0.2, 0.3]), -4.0,
                         n_obs=17, jitter=1e-6)
    state = json.loads(p.to_json())
    assert set(state) == {"data", "cov_func", "metadata"}
    assert state["metadata"]["classname"] == "LandmarksConditionalCholesky"
    assert state["data"]["landmarks"]["type"] == "jax.numpy" and state["data"]["n_obs"] == 17
    assert state["data"]["_state_variables"]["type"] == "set"
    q = m.Predictor.from_dict(state)
    assert isinstance(q, LandmarksConditionalCholesky) and q.n_input_features == 2 and q.mu == -4.0
    assert np.array_equal(q.weights, p.weights) and repr(q.cov_func) == repr(p.cov_func)
    with pytest.raises(ValueError):
        p.mean(np.zeros((2, 3)))                        # feature-count check happens before any device work


def test_shard_bounds_cover_exactly():
    from mellon_amd.distributed import shard_bounds
    for n in (0, 1, 7, 8, 1_000_003):
        for w in (1, 2, 3, 8):
            bounds = [shard_bounds(n, w, r) for r in range(w)]
            assert bounds[0][0] == 0 and bounds[-1][1] == n
            assert all(bounds[i][1] == bounds[i + 1][0] for i in range(w - 1))
            sizes = [b - a for a, b in bounds]
            assert max(sizes) - min(sizes) <= 1


def test_default_tolerance_floor():
    """Why parity is defined against the optimum (inference.LBFGSB_OPTIONS): with the reference's
    stopping rule a 1e-13 relative perturbation of L already moves the answer by > 1e-6, while the
    tight rule is reproducible to < 1e-6 and sits < 1e-3 from the loose answer."""
    x = mo.gaussian_mixture(3000, 8, 7)
    nn = mo.exact_nn_distances(x)
    ref = mo.density_fit(x, n_landmarks=128, nn_distances=nn)
    L, mu = ref.L, ref.mu
    V, Vdr = mo.nn_likelihood_constants(nn, 8)
    rng = np.random.default_rng(0)
    Lq = L * (1 + 1e-13 * rng.normal(size=L.shape))

    def solve(Lm, opts):
        r = mo.minimize_lbfgsb(lambda z: mo.loss_and_grad(z, Lm, mu, V, Vdr), ref.initial_value, opts)
        return Lm @ r.pre_transformation + mu

    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()
    loose = rel(solve(Lq, None), solve(L, None))
    t0, t1 = solve(L, mo.LBFGSB_TIGHT), solve(Lq, mo.LBFGSB_TIGHT)
    assert rel(t1, t0) < 1e-6 < loose
    assert rel(solve(L, None), t0) < 1e-3


def test_bench_prints_exactly_one_stdout_line():
    """bench.py's contract: ONE JSON line on stdout, whatever Python or C-level code prints before or after."""
    import subprocess
    import sys as _sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import os, ctypes, bench\n"
            "real = bench._stdout_to_stderr()\n"
            "print('python noise')\n"
            "ctypes.CDLL(None).puts(b'buffered C noise')\n"
            "os.system('echo child noise')\n"
            "bench._print_result_line(real, '{\"metric\": 1}')\n"
            "print('late python noise')\n"
            "ctypes.CDLL(None).puts(b'late C noise')\n")
    out = subprocess.run([_sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout == '{"metric": 1}\n', out.stdout
    assert "buffered C noise" in out.stderr and "late C noise" in out.stderr


def test_bench_dump_outputs_whole_or_fixed_sample(tmp_path):
    """bench.py --dump-outputs: float64 files; an output within its share of the budget whole, a larger one as the same
    sample of its rows (seed 0, in row order) in every run."""
    import bench
    small = np.arange(10.0)
    big = np.random.default_rng(1).normal(size=(5000, 40)).astype(np.float32)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"small": small, "big": big}, budget=400_000)
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float64 and np.array_equal(s, small)
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float64 and a.shape == (625, 40) and np.array_equal(a, b)
    idx = np.sort(np.random.default_rng(0).choice(5000, 625, replace=False))
    assert np.array_equal(a, big[idx].astype(np.float64))


def test_bench_landmark_cache(tmp_path, monkeypatch):
    """The sklearn landmarks come from the cache on the second call, the same numbers; other cells, another entry."""
    import bench
    from sklearn.cluster import k_means
    monkeypatch.setattr(bench, "LANDMARK_CACHE", str(tmp_path / "cache"))
    x = bench.gaussian_mixture(3000, 6, 11)
    c1, note1 = bench.make_landmarks(x, 40, "sklearn", None)
    assert len(os.listdir(tmp_path / "cache")) == 1 and "cached" not in note1
    c2, note2 = bench.make_landmarks(x, 40, "sklearn", None)
    assert "cached" in note2 and c2.dtype == np.float64 and np.array_equal(c1, c2)
    ref = k_means(x, 40, n_init=1, random_state=42)[0]
    assert np.abs(c1 - ref).max() < 1e-5 * np.abs(ref).max()
    _, note3 = bench.make_landmarks(bench.gaussian_mixture(3000, 6, 12), 40, "sklearn", None)
    assert "cached" not in note3 and len(os.listdir(tmp_path / "cache")) == 2


def test_normalize_per_time_point_validation_and_target_counts():
    """parameter_validation.py:266-280 and parameters.py:436-441 of the reference: dict -> by time value,
    list / array -> by position among the sorted time points, True -> the average count."""
    from mellon_amd.parameter_validation import validate_normalize_parameter
    from mellon_amd.parameters import _target_cell_count
    times = np.array([0.0, 1.5, 4.0])
    validate_normalize_parameter(True, times)
    validate_normalize_parameter([10, 20, 30], times)
    validate_normalize_parameter(np.array([10, 20, 30]), times)
    validate_normalize_parameter({0.0: 10, 1.5: 20, 4.0: 30}, times)
    with pytest.raises(ValueError, match="Missing time point"):
        validate_normalize_parameter({0.0: 10, 1.5: 20}, times)
    with pytest.raises(ValueError, match="must match the number of unique time points"):
        validate_normalize_parameter([10, 20], times)
    with pytest.raises(ValueError, match="must match the number of unique time points"):
        validate_normalize_parameter(np.array([1, 2, 3, 4]), times)
    assert _target_cell_count(True, times[1], 7.0, times) == 7.0
    assert _target_cell_count({0.0: 10, 1.5: 20, 4.0: 30}, times[1], 7.0, times) == 20
    assert _target_cell_count([10, 20, 30], times[2], 7.0, times) == 30
    assert _target_cell_count(np.array([10, 20, 30]), times[0], 7.0, times) == 10


def test_sigma_to_y_cov_factor_reference_cases():
    """The reference's tests/test_sigma_to_y_cov_factor.py:6-43 as data -- scalar, vector and higher-dimensional sigma, and
    the two refusals -- against the product's restatement (mellon_amd/conditional.py) and the oracle's."""
    import numpy as np
    import pytest
    from mellon_amd.conditional import _sigma_to_y_cov_factor as product
    from oracle.mellon_oracle import sigma_to_y_cov_factor as oracle
    for fn in (product, oracle):
        assert np.allclose(fn(0.5, None, 3), np.eye(3) * 0.5)
        assert np.allclose(fn(np.array([1.0, 2.0, 3.0]), None, 3), np.diag([1.0, 2.0, 3.0]))
        got = fn(np.array([[1.0, 2.0], [3.0, 4.0]]), None, 2)
        assert np.allclose(got, np.array([[[1.0, 2.0], [0.0, 0.0]], [[0.0, 0.0], [3.0, 4.0]]]))
        with pytest.raises(ValueError):
            fn(np.array([1.0, 2.0, 3.0]), np.eye(3), 3)
        with pytest.raises(ValueError):
            fn(None, None, 3)
        M = np.arange(6.0).reshape(3, 2)
        assert fn(None, M, 3) is M or np.array_equal(fn(None, M, 3), M)
