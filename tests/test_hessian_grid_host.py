"""PredictorTime._grid_hessian / _grid_hessian_log_determinant with a stub context (no library load): when they decline, what
they hand to the context, how they slice and how they stack blocks of times -- and the longdouble LU the GPU tests measure
against (tests/slogdet_reference.py) checked against numpy here on the CPU."""
import numpy as np
import pytest

import slogdet_reference as sr
from mellon_amd import _lib, cov
from mellon_amd.base_predictor import Predictor, PredictorTime

N, M, D, T = 300, 257, 4, 5


class StubContext:
    """Records the calls; the 'Hessian' of output q at row i is (i + 1000 q) + the entry's position, a d x d pattern whose
    last row and column are recognisable."""
    SLOGDET_MAX_LEAD = _lib.Context.SLOGDET_MAX_LEAD

    def __init__(self):
        self.calls = []

    def leaf_factors(self, leaf, x, y, exact_denominator=True):
        diff = x[:, None, 0] - y[None, :, 0]
        return np.exp(-0.5 * diff ** 2), -np.exp(-0.5 * diff ** 2)

    def predict_mean(self, desc, x, centers, W, mu, out=None):
        self.calls.append(("mean", desc, x, np.array(W)))
        return np.zeros((x.shape[0], W.shape[1]))

    def predict_hessian(self, desc, x, centers, W):
        self.calls.append(("hessian", desc, x, np.array(W)))
        n, d = x.shape
        tag = W[0] if W.ndim == 2 else W[:1]                       # the stub weights carry the time index in row 0
        return (np.arange(n)[:, None, None, None] + 1000.0 * tag[None, :, None, None]
                + np.arange(d * d, dtype=float).reshape(1, 1, d, d) / 100.0)

    def predict_hessian_logdet(self, desc, x, centers, W, lead=None):
        self.calls.append(("logdet", desc, x, np.array(W), lead))
        shape = (x.shape[0],) + W.shape[1:]
        return np.ones(shape), np.zeros(shape)


@pytest.fixture
def stub(monkeypatch):
    s = StubContext()
    monkeypatch.setattr(_lib, "default_context", lambda: s)
    return s


def _tree():
    return cov.Matern52(1.7, active_dims=slice(None, -1)) * cov.ExpQuad(0.9, active_dims=-1)


def _predictor(tree=None, weights=None, m=M):
    rng = np.random.default_rng(0)
    c = rng.normal(size=(m, D))
    w = rng.normal(size=m) if weights is None else weights
    return PredictorTime(_tree() if tree is None else tree, c, w, 0.3)


X = np.random.default_rng(1).normal(size=(N, D - 1))
TS = np.linspace(0.0, 1.0, T)

DECLINING = {
    "one time": lambda: (_predictor(), X, TS[:1]),
    "2-D weights": lambda: (_predictor(weights=np.ones((M, 2))), X, TS),
    "a tree that does not split": lambda: (_predictor(cov.Matern52(1.7, active_dims=slice(None, -1))
                                                      + cov.ExpQuad(0.9, active_dims=-1)), X, TS),
    "less work than the loop's threshold": lambda: (_predictor(m=3), X[:4], TS),
}


@pytest.mark.parametrize("case", sorted(DECLINING))
def test_the_grids_decline_where_grid_setup_does(stub, case):
    pt, x, ts = DECLINING[case]()
    assert pt._grid_setup(x, ts) is None
    assert pt._grid_hessian(x, times=ts) is NotImplemented
    assert pt._grid_hessian_log_determinant(x, times=ts) is NotImplemented
    assert not [c for c in stub.calls if c[0] in ("hessian", "logdet")]


def test_device_resident_queries_decline(stub):
    class FakeDeviceArray(_lib.DeviceArray):
        def __init__(self):
            pass
    pt = _predictor()
    assert pt._grid_hessian(FakeDeviceArray(), times=TS) is NotImplemented
    assert pt._grid_hessian_log_determinant(FakeDeviceArray(), times=TS) is NotImplemented


def test_the_weights_are_those_of_the_grid_mean_and_the_state_columns_are_kept(stub):
    pt = _predictor()
    pt._grid_mean(X, times=TS)
    H = pt._grid_hessian(X, times=TS)
    sign, logabs = pt._grid_hessian_log_determinant(X, times=TS)
    mean, hess, logdet = stub.calls
    assert (mean[0], hess[0], logdet[0]) == ("mean", "hessian", "logdet")
    E = mean[3]
    assert E.shape == (M, T) and np.array_equal(hess[3], E) and np.array_equal(logdet[3], E)
    K, _ = stub.leaf_factors(None, TS.reshape(-1, 1), pt.centers[:, -1:])
    assert np.array_equal(E, (K * pt.weights).T)
    for call in (hess, logdet):                       # the state program over all d columns, queries [x | 0]
        assert [tuple(leaf[3]) for leaf in call[1].leaves] == [tuple(range(D - 1))]
        assert call[2].shape == (N, D) and np.array_equal(call[2][:, :-1], X) and not call[2][:, -1].any()
    assert logdet[4] == D - 1 and sign.shape == logabs.shape == (N, T)
    full = stub.predict_hessian(None, hess[2], None, E)
    assert H.shape == (N, T, D - 1, D - 1) and H.flags.c_contiguous and np.array_equal(H, full[..., :-1, :-1])


def test_blocks_of_times_are_stacked_in_order(stub, monkeypatch):
    """A host bound of two times' worth of (n, d, d) results: blocks of 2, 2 and 1 times, each in its place."""
    pt = _predictor()
    tagged = np.zeros((M, T))
    tagged[0] = np.arange(T)                           # what the stub reads the time index from
    monkeypatch.setattr(PredictorTime, "_grid_setup",
                        lambda self, x, times, want_derivative=False: ("state", np.column_stack([x, np.zeros(len(x))]),
                                                                       tagged, None))
    whole = pt._grid_hessian(X, times=TS)
    assert [c[3].shape for c in stub.calls] == [(M, T)]
    del stub.calls[:]
    monkeypatch.setattr(PredictorTime, "_GRID_HESSIAN_DOUBLES", 2 * N * D * D)
    blocked = pt._grid_hessian(X, times=TS)
    assert [c[3].shape for c in stub.calls] == [(M, 2), (M, 2), (M, 1)]
    assert [c[3][0].tolist() for c in stub.calls] == [[0.0, 1.0], [2.0, 3.0], [4.0]]
    assert blocked.shape == (N, T, D - 1, D - 1) and np.array_equal(blocked, whole)
    assert np.array_equal(blocked[5, :, 0, 0], 5 + 1000.0 * np.arange(T))
    monkeypatch.setattr(PredictorTime, "_GRID_HESSIAN_DOUBLES", 1)             # never less than one time per call
    del stub.calls[:]
    assert np.array_equal(pt._grid_hessian(X, times=TS), whole) and len(stub.calls) == T


def test_a_state_block_the_device_does_not_factor_takes_the_loop(stub):
    d = _lib.Context.SLOGDET_MAX_LEAD + 2
    c = np.random.default_rng(2).normal(size=(M, d))
    pt = PredictorTime(_tree(), c, np.ones(M), 0.0)
    x = np.zeros((N, d - 1))
    assert pt._grid_hessian_log_determinant(x, times=TS) is NotImplemented
    assert pt._grid_hessian(x, times=TS).shape == (N, T, d - 1, d - 1)


def test_the_fused_entry_is_for_predictors_own_hessian_above_the_threshold(stub, monkeypatch):
    from mellon_amd.base_predictor import ExpPredictor
    rng = np.random.default_rng(3)
    c, w = rng.normal(size=(M, D)), rng.normal(size=M)
    x = rng.normal(size=(N, D))
    sign, _ = Predictor(cov.Matern52(1.7), c, w, 0.0).hessian_log_determinant(x)
    assert [(call[0], call[4]) for call in stub.calls] == [("logdet", D)] and sign.shape == (N,)
    del stub.calls[:]
    Predictor(cov.Matern52(1.7), c, w, 0.0).hessian_log_determinant(x[:20])    # 20 x 257 pairs: the host path
    assert [call[0] for call in stub.calls] == ["hessian"]
    del stub.calls[:]
    monkeypatch.setattr(ExpPredictor, "hessian", lambda self, x, jit=True: np.tile(np.eye(D), (len(x), 1, 1)))
    sign, logabs = ExpPredictor(cov.Matern52(1.7), c, w, 0.0).hessian_log_determinant(x)
    assert not stub.calls and np.array_equal(sign, np.ones(N)) and np.array_equal(logabs, np.zeros(N))
    _predictor().hessian_log_determinant(X, time=0.5)                          # PredictorTime, one time: the state block
    assert [(call[0], call[4]) for call in stub.calls] == [("logdet", D - 1)]


@pytest.mark.parametrize("k", [1, 2, 3, 8, 31])
def test_the_longdouble_lu_agrees_with_numpy(k):
    for name, (A, singular) in sr.crafted(k, count=12).items():
        sign, logabs = sr.slogdet_longdouble(A)
        if singular:
            assert np.array_equal(sign, np.zeros(len(A))) and np.all(logabs == -np.inf), name
            continue
        s_np, l_np = np.linalg.slogdet(A)
        assert np.array_equal(sign, s_np), name
        assert np.abs(logabs.astype(np.float64) - l_np).max() < 1e-11, name
        assert np.linalg.cond(A).max() <= sr.COND_MAX or name == "odd permutation"
    # exact values: a diagonal of powers of two and a row swap
    A = np.diag([2.0, -4.0, 0.5])[[1, 0, 2]][None]
    sign, logabs = sr.slogdet_longdouble(A)
    assert sign[0] == 1.0 and abs(logabs[0] - np.log(np.longdouble(4.0))) < 1e-18
    e_dev, e_lap, bound = sr.logdet_errors(A, np.linalg.slogdet(A)[1])
    assert e_dev == e_lap and bound == 4.0 * e_lap + 9 * sr.EPS
