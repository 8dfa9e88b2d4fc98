"""Host-only logic of the cell-sharded FunctionEstimator (no GPU): thread-ranks over the product's ThreadHostComm with no
device context.  Everything checked here happens BEFORE the first device call of a fit -- the decisions from global
counts, the input errors agreed on by all ranks, the refusal of the full GP -- so the real `fit` runs up to its error."""
import os
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _run_ranks(world, body):
    """body(rank, comm) on `world` thread-ranks; returns per rank the value or the exception it raised.  A rank that
    raises does NOT release the others (no barrier abort): a check that only one rank made would hang the join, which
    the deadline below turns into a failure."""
    from mellon_amd import distributed
    group = distributed.ThreadGroup(world)
    out = [None] * world

    def run(rank):
        comm = distributed.ShardedCommunicator(None, distributed.ThreadHostComm(group, rank))
        distributed.set_thread_current(comm)
        try:
            out[rank] = body(rank, comm)
        except BaseException as e:     # noqa: BLE001 -- the result of this rank
            out[rank] = e
        finally:
            distributed.set_thread_current(None)

    threads = [threading.Thread(target=run, args=(r,), daemon=True) for r in range(world)]
    [t.start() for t in threads]
    [t.join(60) for t in threads]
    assert not any(t.is_alive() for t in threads), "a rank is still waiting in a collective: the ranks did not act together"
    return out


def _cells(n=1200, d=3, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, d))
    return x, np.sin(x[:, :2]) + 0.1 * rng.normal(size=(n, 2))


def _shard(a, world, rank):
    from mellon_amd.distributed import shard_bounds
    lo, hi = shard_bounds(a.shape[0], world, rank)
    return np.ascontiguousarray(a[lo:hi])


def test_decisions_come_from_the_global_count():
    """3 shards of 400 cells, n_landmarks = 500: a shard alone would resolve to the full GP."""
    import mellon_amd
    from mellon_amd.util import GaussianProcessType
    x, _ = _cells()

    def body(rank, comm):
        est = mellon_amd.FunctionEstimator(n_landmarks=500, sigma=0.3)
        est.set_x(_shard(x, 3, rank))
        est._prepare_attribute("n_landmarks")
        est._prepare_attribute("gp_type")
        est.validate_parameter()
        default = mellon_amd.FunctionEstimator(sigma=0.3)
        default.set_x(_shard(x, 3, rank))
        return est.n_landmarks, est.gp_type, est._n_cells_global(), default._compute_n_landmarks()

    assert _run_ranks(3, body) == [(500, GaussianProcessType.SPARSE_CHOLESKY, 1200, 1200)] * 3
    one = mellon_amd.FunctionEstimator(n_landmarks=500, sigma=0.3)
    one.set_x(_shard(x, 3, 1))
    assert one._compute_gp_type() == GaussianProcessType.FULL       # what the base class's local decision gives


def test_ls_is_the_single_rank_value_bit_for_bit():
    """400-cell shards do not line up with NumPy's pairwise summation: a sum of partial sums would differ in the last
    bits, the gathered sum does not."""
    import mellon_amd
    nn = np.abs(np.random.default_rng(5).normal(size=1200)) + 0.01
    one = mellon_amd.FunctionEstimator(nn_distances=nn, ls_factor=1.7)
    want = one._compute_ls()

    def body(rank, comm):
        return mellon_amd.FunctionEstimator(nn_distances=_shard(nn, 3, rank), ls_factor=1.7)._compute_ls()

    assert _run_ranks(3, body) == [want] * 3


@pytest.mark.parametrize("kw", [dict(), dict(gp_type="full")])
def test_full_gp_is_refused_on_every_rank(kw):
    """300 cells: the defaults resolve to the full GP from the GLOBAL count (n_landmarks = 300 >= 300)."""
    import mellon_amd
    x, y = _cells(300)
    out = _run_ranks(3, lambda rank, comm: mellon_amd.FunctionEstimator(sigma=0.3, **kw).fit(_shard(x, 3, rank), _shard(y, 3, rank)))
    assert all(isinstance(e, NotImplementedError) for e in out), out
    assert all("full Gaussian process of the FunctionEstimator" in str(e) for e in out)


class _BrokenCSR:
    """A sparse container whose CSR arrays do not describe its shape."""
    shape = (400, 2)

    def todense(self):
        raise AssertionError("sparse targets must not be made dense")

    def tocsr(self):
        return self

    indptr = np.arange(401, dtype=np.int64)
    indices = np.full(400, 7, dtype=np.int32)       # column 7 of 2
    data = np.ones(400)


def _bad_inputs():
    x, y = _cells()
    nan_y = y.copy()
    nan_y[500, 1] = np.nan
    sig = np.full(1200, 0.3)
    sig[450] = 0.0
    return {
        "length": (dict(sigma=0.3), lambda r: _shard(y, 3, r)[:-1] if r == 1 else _shard(y, 3, r), "should equal y.shape"),
        "non-finite": (dict(sigma=0.3), lambda r: _shard(nan_y, 3, r), "non-finite"),
        "sigma<=0": (dict(sigma=sig), lambda r: _shard(y[:, 0], 3, r), "sigma must be positive"),
        "sigma shape": (dict(sigma=np.full(7, 0.3)), lambda r: _shard(y, 3, r), "Unsupported sigma configuration"),
        "csr": (dict(sigma=0.3), lambda r: _BrokenCSR() if r == 1 else _shard(y, 3, r), "not a valid CSR matrix"),
    }


@pytest.mark.parametrize("case", ["length", "non-finite", "sigma<=0", "sigma shape", "csr"])
def test_input_errors_of_one_rank_are_raised_by_all(case):
    """Each error sits in rank 1's rows (the sigma shape in everybody's); all three ranks raise the same ValueError, and
    nobody is left waiting (the per-cell sigma is sharded with the cells)."""
    import mellon_amd
    x, _ = _cells()
    kw, y_of, text = _bad_inputs()[case]

    def body(rank, comm):
        kw_r = dict(kw)
        if np.ndim(kw_r["sigma"]) == 1 and kw_r["sigma"].shape[0] == 1200:
            kw_r["sigma"] = _shard(kw_r["sigma"], 3, rank)
        return mellon_amd.FunctionEstimator(n_landmarks=50, **kw_r).fit(_shard(x, 3, rank), y_of(rank))

    out = _run_ranks(3, body)
    assert all(isinstance(e, ValueError) for e in out), out
    assert len({str(e) for e in out}) == 1 and text in str(out[0]), out
    if case != "sigma shape":
        assert "1 of 3 ranks" in str(out[0]) and "rank 1:" in str(out[0])


def test_an_empty_shard_is_refused_on_every_rank():
    import mellon_amd
    x, y = _cells(90)
    cuts = [0, 50, 50, 90]
    out = _run_ranks(3, lambda r, comm: mellon_amd.FunctionEstimator(n_landmarks=10, sigma=0.3).fit(
        np.ascontiguousarray(x[cuts[r]:cuts[r + 1]]), np.ascontiguousarray(y[cuts[r]:cuts[r + 1]])))
    assert all(isinstance(e, ValueError) for e in out), out
    assert len({str(e) for e in out}) == 1 and "[50, 0, 40]" in str(out[0]) and "ranks [1] hold no cells" in str(out[0])


def test_single_rank_errors_are_what_they_were():
    import mellon_amd
    x, y = _cells(60)
    with pytest.raises(ValueError, match=r"^X.shape\[0\] = 60 \(n_samples\) should equal y.shape\[0\] = 59\.$"):
        mellon_amd.FunctionEstimator(sigma=0.3).fit(x, y[:-1])


def test_leverage_gram_is_formed_over_the_gathered_points_without_a_collective(monkeypatch):
    """Shards of 70,000 and 10 query rows (mln_kernel_gram would all-reduce twice on one rank, once on the other):
    every rank makes ONE call, on a context of its own that belongs to no communicator, with the points of all
    ranks in rank order -- the single-rank call, hence the single-rank bits."""
    from mellon_amd import _lib, conditional
    rows = [70_000, 10]
    rng = np.random.default_rng(1)
    xs = [rng.normal(size=(n, 4)) for n in rows]
    made = []

    class Solo:
        handle = 1

        def __init__(self, device):
            self.device, self.calls = device, []
            made.append(self)

        def kernel_gram(self, desc, x, xu):
            self.calls.append(x.shape[0])
            return x.T @ x

    class RankCtx:
        device = 3

        def kernel_gram(self, desc, x, xu):
            raise AssertionError("the rank's own context would all-reduce")

    monkeypatch.setattr(_lib, "Context", Solo)

    def body(rank, comm):
        ctx = RankCtx()
        first = conditional._kernel_gram_all_ranks(ctx, None, xs[rank], np.zeros((4, 4)))
        again = conditional._kernel_gram_all_ranks(ctx, None, xs[rank], np.zeros((4, 4)))
        return first, again, ctx._solo

    out = _run_ranks(2, body)
    x_all = np.concatenate(xs)
    assert len(made) == 2 and all(c.device == 3 and c.calls == [70_010, 70_010] for c in made)      # one context per rank, reused
    for first, again, _ in out:
        assert np.array_equal(first, x_all.T @ x_all) and np.array_equal(again, first)

    class One:                                                        # single rank: the one call there always was
        calls = []

        def kernel_gram(self, desc, x, xu):
            self.calls.append(x.shape[0])
            return x.T @ x

    conditional._kernel_gram_all_ranks(One(), None, xs[0], np.zeros((4, 4)))
    assert One.calls == [70_000] and len(made) == 2
