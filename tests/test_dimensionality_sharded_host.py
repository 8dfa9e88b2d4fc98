"""Host-only logic of the cell-sharded DimensionalityEstimator (no GPU): the duplicate-cell counts are summed over the
ranks so that every rank raises the same error (a `gloo` world of 2, as tests/test_distributed_cpu.py builds it), and
the k-NN layer searches this rank's cells among the cells of all ranks with k validated against the global count
(two thread-ranks over the product's ThreadHostComm, the device search replaced by a NumPy one)."""
import os
import socket
import sys
import threading

import numpy as np
import pytest

import dim_restatement as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gloo_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import mellon_amd
    from mellon_amd import distributed
    from mellon_amd.dimensionality_estimator import _count_over_ranks

    class GlooHostComm(distributed.HostComm):
        def allgather(self, obj):
            out = [None] * world
            dist.all_gather_object(out, obj)
            return out

    host = GlooHostComm()
    host.rank, host.world_size = rank, world
    distributed.set_current(distributed.ShardedCommunicator(None, host))
    assert _count_over_ranks(3 if rank == 0 else 0) == 3
    assert _count_over_ranks(np.int64(rank + 1)) == 3

    rng = np.random.default_rng(rank)
    # rank 1 alone holds zero distances: BOTH ranks raise, naming the global count
    dist_rows = np.sort(np.abs(rng.normal(size=(7 + rank, 10))) + 0.1, axis=1)
    if rank == 1:
        dist_rows[[0, 3, 5], 0] = 0.0
    est = mellon_amd.DimensionalityEstimator(distances=dist_rows)
    with pytest.raises(ValueError, match="^3 cells have a nearest-neighbour distance of 0"):
        est._compute_nn_distances()
    # no zero anywhere: this rank's column
    clean = mellon_amd.DimensionalityEstimator(distances=np.maximum(dist_rows, 0.05))
    assert np.array_equal(clean._compute_nn_distances(), np.maximum(dist_rows, 0.05)[:, 0])
    with open(os.path.join(out_dir, f"ok{rank}"), "w") as fh:
        fh.write("ok")
    dist.destroy_process_group()


def test_duplicate_count_is_summed_over_a_gloo_world_of_two(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_gloo_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    assert sorted(os.listdir(tmp_path)) == ["ok0", "ok1"]


def test_single_rank_count_and_message_are_unchanged():
    sys.path.insert(0, ROOT)
    import mellon_amd
    from mellon_amd.dimensionality_estimator import _count_over_ranks
    assert _count_over_ranks(np.int64(4)) == 4 and isinstance(_count_over_ranks(np.int64(4)), int)
    rows = np.ones((5, 3))
    rows[1:3, 0] = 0.0
    with pytest.raises(ValueError, match="^2 cells have a nearest-neighbour distance of 0"):
        mellon_amd.DimensionalityEstimator(distances=rows)._compute_nn_distances()


class _NumpyCtx:
    """The two device calls of the k-NN layer, restated in NumPy (ties: smaller index first)."""

    def knn(self, x, k, y=None, exclude_self=False, self_offset=0, return_index=True):
        y = x if y is None else y
        d2 = ((x[:, None, :] - y[None, :, :]) ** 2).sum(-1)
        if exclude_self:
            d2[np.arange(x.shape[0]), np.arange(x.shape[0]) + self_offset] = np.inf
        idx = np.argsort(d2, axis=1, kind="stable")[:, :k]
        dist = np.sqrt(np.take_along_axis(d2, idx, axis=1))
        return (dist, idx.astype(np.int64)) if return_index else dist

    def local_dimensionality(self, x, neighbor_idx):
        return dr.local_dimensionality(x, neighbor_idx=neighbor_idx)


@pytest.mark.parametrize("k", [5, 40, 64])
def test_knn_layer_searches_own_cells_among_all_cells(monkeypatch, k):
    """k + 1 <= 30, 30 < k + 1 <= 64 and k = 64; the second shard holds 3 cells, fewer than any k here."""
    sys.path.insert(0, ROOT)
    import mellon_amd
    from mellon_amd import _lib, distributed
    monkeypatch.setattr(_lib, "default_context", lambda: _NumpyCtx())
    rng = np.random.default_rng(6)
    n = 90
    x = rng.normal(size=(n, 3))
    cuts = [0, 50, 53, n]
    ctx = _NumpyCtx()
    want = ctx.knn(x, k, exclude_self=True, return_index=False)
    want_d = dr.local_dimensionality(x)
    group = distributed.ThreadGroup(3)
    out, errs = [None] * 3, []

    def body(rank):
        try:
            distributed.set_thread_current(distributed.ShardedCommunicator(None, distributed.ThreadHostComm(group, rank)))
            lo, hi = cuts[rank], cuts[rank + 1]
            est = mellon_amd.DimensionalityEstimator(k=k)
            est.set_x(np.ascontiguousarray(x[lo:hi]))
            distances = est._compute_distances()
            idx = est._knn_idx[1].copy()
            d = est._compute_d()
            too_many = mellon_amd.DimensionalityEstimator(k=64)
            too_many.set_x(np.ascontiguousarray(x[lo:lo + 20 * (rank + 1)][:hi - lo]))      # 20 + 3 + 37 = 60 cells
            with pytest.raises(ValueError, match="k=64 must be smaller than the number of samples 60"):
                too_many._compute_distances()
            out[rank] = (distances, idx, d)
        except BaseException as e:     # noqa: BLE001
            errs.append(e)
            group.barrier.abort()
        finally:
            distributed.set_thread_current(None)

    ts = [threading.Thread(target=body, args=(r,)) for r in range(3)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    for rank, (distances, idx, d) in enumerate(out):
        lo, hi = cuts[rank], cuts[rank + 1]
        assert distances.shape == (hi - lo, k)
        np.testing.assert_allclose(distances, want[lo:hi], rtol=1e-13)
        assert idx.shape == (hi - lo, 30) and np.array_equal(idx[:, 0], np.arange(lo, hi))      # global indices
        np.testing.assert_allclose(d, want_d[lo:hi], rtol=1e-10)


def test_non_finite_local_dimension_count_is_global(monkeypatch):
    """A cell of rank 0 repeated on rank 1: the zero pair distance sits in neighbourhoods on both ranks, and both raise
    the count a single rank would."""
    sys.path.insert(0, ROOT)
    import mellon_amd
    from mellon_amd import _lib, distributed
    monkeypatch.setattr(_lib, "default_context", lambda: _NumpyCtx())
    rng = np.random.default_rng(2)
    x = rng.normal(size=(80, 2))
    x[70] = x[4]
    bad = int(np.count_nonzero(~np.isfinite(dr.local_dimensionality(x))))
    assert bad >= 2
    group = distributed.ThreadGroup(2)
    out = [None, None]

    def body(rank):
        try:
            distributed.set_thread_current(distributed.ShardedCommunicator(None, distributed.ThreadHostComm(group, rank)))
            est = mellon_amd.DimensionalityEstimator(distances=np.ones((40, 10)))
            est.set_x(np.ascontiguousarray(x[40 * rank:40 * rank + 40]))
            est._compute_d()
        except ValueError as e:
            out[rank] = str(e)
        except BaseException as e:     # noqa: BLE001
            out[rank] = e
            group.barrier.abort()
        finally:
            distributed.set_thread_current(None)

    ts = [threading.Thread(target=body, args=(r,)) for r in range(2)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert out[0] == out[1] and isinstance(out[0], str), out
    assert out[0].startswith(f"{bad} cells have a non-finite local dimension"), out[0]
