"""Host-only logic of the automatic `ls_time` on cell-sharded input (no GPU): the two-pass correlation from all-reduced
sums, the global list of time points, the gather of one time point in global order and its re-shard bounds -- thread-ranks
over the product's ThreadHostComm, tables in NumPy."""
import os
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _run_ranks(world, fn):
    """fn(comm) on `world` thread-ranks joined by a ThreadHostComm; results in rank order."""
    from mellon_amd import distributed
    group = distributed.ThreadGroup(world)
    out, errs = [None] * world, []

    def body(rank):
        try:
            out[rank] = fn(distributed.ShardedCommunicator(None, distributed.ThreadHostComm(group, rank)))
        except BaseException as e:     # noqa: BLE001 -- reported below
            errs.append(e)
            group.barrier.abort()

    ts = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    if errs:
        raise errs[0]
    return out


@pytest.mark.parametrize("cuts", [[0, 1400, 3001], [0, 7, 1999, 3001]], ids=["2 ranks", "3 ranks"])
def test_sharded_correlation_equals_corrcoef(cuts):
    """T = 4 rows of n = 3001 columns spread unevenly over 2 and 3 ranks.  Entries of a correlation lie in [-1, 1]; the
    only difference to np.corrcoef of the whole table is the re-association of sums of ~3e3 fp64 terms (~3e-13), so
    1e-11 absolute; and every rank holds the same bits."""
    from mellon_amd.compute_ls_time import HostTable, correlation_of_rows_sharded
    rng = np.random.default_rng(3)
    base = rng.normal(size=3001)
    # log-density-like rows: a large common offset (what a one-pass formula would cancel on) and partial correlation
    table = np.stack([-40.0 + 3.0 * (w * base + (1 - w) * rng.normal(size=3001)) for w in (1.0, 0.8, 0.5, 0.1)])
    want = np.corrcoef(table)
    world = len(cuts) - 1

    def body(comm):
        local = np.array(table[:, cuts[comm.rank]:cuts[comm.rank + 1]])
        return correlation_of_rows_sharded(HostTable(local), comm.allreduce_sum)

    got = _run_ranks(world, body)
    for g in got:
        assert g.shape == (4, 4)
        assert np.array_equal(g, got[0])
        assert np.abs(g - want).max() <= 1e-11, np.abs(g - want).max()


def test_sharded_correlation_with_a_rank_that_holds_no_column():
    from mellon_amd.compute_ls_time import HostTable, correlation_of_rows_sharded
    rng = np.random.default_rng(4)
    table = rng.normal(size=(3, 50)) + 10.0
    cuts = [0, 50, 50]
    got = _run_ranks(2, lambda comm: correlation_of_rows_sharded(
        HostTable(np.array(table[:, cuts[comm.rank]:cuts[comm.rank + 1]])), comm.allreduce_sum))
    assert np.array_equal(got[0], got[1])
    assert np.abs(got[0] - np.corrcoef(table)).max() <= 1e-12


def test_global_time_points_and_gather_when_ranks_miss_time_points():
    """Rows sorted by time, contiguous shards: rank 0 holds only time point 0.5, rank 2 only 3.0 and 7.25, rank 3 no cell
    at all.  Every rank gets the sorted union, and each time point's cells arrive in global order."""
    from mellon_amd.compute_ls_time import gather_time_point, global_time_points
    rng = np.random.default_rng(5)
    stamp = np.repeat([0.5, 1.0, 3.0, 7.25], [9, 4, 6, 2])
    states = rng.normal(size=(stamp.size, 3))
    nn = rng.uniform(0.1, 1.0, size=stamp.size)
    cuts = [0, 7, 15, 21, 21]

    def body(comm):
        lo, hi = cuts[comm.rank], cuts[comm.rank + 1]
        s, st, d = states[lo:hi], stamp[lo:hi], nn[lo:hi]
        stamps = global_time_points(comm.host, st)
        return stamps, [gather_time_point(comm.host, s, st, d, t) for t in stamps]

    for stamps, gathered in _run_ranks(4, body):
        assert np.array_equal(stamps, [0.5, 1.0, 3.0, 7.25]) and stamps.dtype == np.float64
        for t, (x_t, nn_t) in zip(stamps, gathered):
            assert np.array_equal(x_t, states[stamp == t]) and np.array_equal(nn_t, nn[stamp == t])
            assert x_t.flags.c_contiguous and x_t.shape[1] == 3


@pytest.mark.parametrize("n_t,world", [(10, 3), (11, 4), (7, 7), (1200, 3), (1501, 2)])
def test_reshard_bounds_cover_the_time_point(n_t, world):
    from mellon_amd.compute_ls_time import reshard_bounds
    bounds = [reshard_bounds(n_t, world, r, 1.0) for r in range(world)]
    assert bounds[0][0] == 0 and bounds[-1][1] == n_t
    assert all(a[1] == b[0] for a, b in zip(bounds[:-1], bounds[1:]))
    sizes = [hi - lo for lo, hi in bounds]
    assert min(sizes) >= 1 and max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)


def test_fewer_cells_than_ranks_is_one_value_error_on_every_rank():
    from mellon_amd.compute_ls_time import reshard_bounds
    messages = set()
    for rank in range(4):
        with pytest.raises(ValueError, match=r"Time point 2\.5 has 3 cells but the fit runs on 4 ranks") as err:
            reshard_bounds(3, 4, rank, 2.5)
        messages.add(str(err.value))
    assert len(messages) == 1
