"""Length scale of the time axis for TimeSensitiveDensityEstimator when `ls_time` is not given
(reference: mellon/compute_ls_time.py:12-105).

Idea of the reference: fit one density per time point, evaluate every one of them on ALL cells, and pick the kernel
length scale whose covariance over the time gaps |t_a - t_b| best matches (Frobenius norm) the correlation of those
log-densities.  Here the per-time-point fits and their cross-evaluation are device work (each fit is the hot path on
that time point's cells; each evaluation one fused predict pass), the T x T correlation and the one-dimensional
search are host arithmetic on a handful of numbers.  `compute_ls_time_sharded` (second half of this file) is the
same algorithm for cells sharded across ranks; `compute_ls_time` itself is the single-rank path.
"""
import logging

import numpy as np
from scipy.optimize import minimize

from .density_estimator import DensityEstimator
from .parameter_validation import validate_params
from .parameters import compute_gp_type, compute_n_landmarks
from .util import GaussianProcessType
from .validation import validate_time_x

logger = logging.getLogger("mellon")

SMALL_TIME_POINT = 500      # cells below which the reference warns about an unreliable time point


def _fit_time_points(states, stamp, nn_distances, estimator_kwargs):
    """One DensityEstimator per distinct time stamp, fitted on that time point's cells only.
    Returns (sorted unique stamps, fitted estimators)."""
    stamps = np.unique(stamp)
    fitted = []
    for rank, t in enumerate(stamps, start=1):
        members = np.flatnonzero(stamp == t)
        logger.info(f"[{rank} of {len(stamps)}] Computing density for {members.size:,} cells at time point {t}.")
        if members.size < SMALL_TIME_POINT:
            logger.warning(f"Time point {t} only has {members.size:,} cells. "
                           "This could lead to inaccurate estimation of the time length scale `ls_time`.")
        model = DensityEstimator(nn_distances=nn_distances[members], **estimator_kwargs)
        model.fit(np.ascontiguousarray(states[members]))
        fitted.append(model)
    return stamps, fitted


def _correlation_of_rows(table):
    """Pearson correlation between the rows of `table` (T x n): centred rows, normalised Gram."""
    centred = table - table.mean(axis=1, keepdims=True)
    gram = centred @ centred.T
    scale = np.sqrt(np.diag(gram))
    return gram / np.outer(scale, scale)


def _closest_length_scale(cov_func_curry, stamps, target):
    """argmin over ls of || k_ls(|t_a - t_b|) - target ||_F, searched in log ls from ls = 1 with L-BFGS-B (the
    reference's jaxopt.ScipyMinimize(method="L-BFGS-B").run(0.0); the derivative comes from differences here).
    The kernel is evaluated on the DISTINCT gaps only and scattered into the T x T matrix."""
    gaps = np.abs(stamps[:, None] - stamps[None, :])
    distinct, where = np.unique(gaps, return_inverse=True)
    where = where.reshape(gaps.shape)
    column, origin = distinct.reshape(-1, 1), np.zeros((1, 1))

    def misfit(log_ls):
        kernel = cov_func_curry(float(np.exp(np.ravel(log_ls)[0])))
        values = np.asarray(kernel(column, origin)).reshape(-1)
        return float(np.linalg.norm(values[where] - target))

    found = minimize(misfit, np.zeros(1), method="L-BFGS-B")
    return float(np.exp(found.x[0]))


def compute_ls_time(nn_distances, x, cov_func_curry, times=None, warn_below=SMALL_TIME_POINT, return_data=False,
                    density_estimator_kwargs=None):
    """ls_time, or with `return_data` the tuple (ls_time, densities [T x n], per-time-point estimators, time points)."""
    global SMALL_TIME_POINT
    xt = np.asarray(validate_time_x(x, times), dtype=np.float64)
    states, stamp = np.ascontiguousarray(xt[:, :-1]), xt[:, -1]
    nn_distances = np.asarray(nn_distances, dtype=np.float64)
    previous, SMALL_TIME_POINT = SMALL_TIME_POINT, warn_below
    try:
        stamps, fitted = _fit_time_points(states, stamp, nn_distances, dict(density_estimator_kwargs or {}))
    finally:
        SMALL_TIME_POINT = previous
    # every time point's density evaluated on the cells of ALL time points (one fused device pass each)
    table = np.stack([model.predict(states) for model in fitted])
    ls_time = _closest_length_scale(cov_func_curry, stamps, _correlation_of_rows(table))
    if return_data:
        return ls_time, table, fitted, stamps
    return ls_time


# ---- cells sharded across ranks ------------------------------------------------------------------------------------
# The same algorithm when every rank holds a contiguous block of the cells.  What makes it rank-safe:
#   * every rank walks the SAME list of time points (the sorted union of the ranks' stamps);
#   * a time point is fitted on its cells of ALL ranks, gathered in global order and dealt out again in equal
#     contiguous slices -- input sorted by time would otherwise leave most ranks without a cell of it;
#   * the correlation is taken over the cells of all ranks from all-reduced sums (T + 1, then T x T numbers);
#   * the one-dimensional search runs on identical input everywhere and rank 0's result is broadcast.


def global_time_points(host, stamp):
    """The sorted distinct time stamps of the cells of all ranks (`host`: the ranks' host communicator); a rank that
    holds no cell of some time point, or no cell at all, still receives the full list."""
    local = np.unique(np.asarray(stamp, dtype=np.float64).reshape(-1))
    return np.unique(np.concatenate(host.allgather(local)))


def gather_time_point(host, states, stamp, nn_distances, t):
    """(cells, nn distances) of time point t over all ranks, in global cell order -- the order of states[members] on
    one rank, because the ranks hold contiguous blocks and are gathered in rank order."""
    members = np.flatnonzero(stamp == t)
    parts = host.allgather((np.ascontiguousarray(states[members]), np.ascontiguousarray(nn_distances[members])))
    return (np.ascontiguousarray(np.concatenate([p[0] for p in parts], axis=0)),
            np.ascontiguousarray(np.concatenate([p[1] for p in parts])))


def reshard_bounds(n_t, world_size, rank, t=None):
    """This rank's [start, stop) of the n_t gathered cells of a time point (distributed.shard_bounds).  Every rank must
    receive a cell: the nested fit has no legal empty shard, so fewer cells than ranks is one ValueError, raised from
    global counts and therefore on every rank alike."""
    from .distributed import shard_bounds
    if n_t < world_size:
        raise ValueError(f"Time point {t} has {n_t:,} cells but the fit runs on {world_size:,} ranks: the automatic "
                         "`ls_time` fits every time point on all ranks and needs at least one cell per rank. Pass "
                         "`ls_time=` or use fewer ranks.")
    return shard_bounds(n_t, world_size, rank)


class HostTable:
    """The three operations the sharded correlation needs, on a NumPy T x n_local table (changed in place)."""

    def __init__(self, table):
        self.table = np.asarray(table, dtype=np.float64)
        self.shape = self.table.shape

    def row_sums(self):
        return self.table.sum(axis=1)

    def centre(self, means):
        self.table -= np.asarray(means, dtype=np.float64)[:, None]

    def gram(self):
        return self.table @ self.table.T


class DeviceTable:
    """The same three operations on a T x n_local table in HBM: the row sums and the Gram are one skinny fp64 GEMM each
    (mln_gemm), the centring one element-wise pass per row; only T and T x T numbers come back."""

    def __init__(self, ctx, table):
        self.ctx, self.table, self.shape = ctx, table, tuple(table.shape)

    def row_sums(self):
        T, n = self.shape
        ones = self.ctx.to_device(np.ones((n, 1)))
        try:
            return self.ctx.gemm(self.table, ones, out=np.empty((T, 1))).reshape(-1)
        finally:
            ones.free()

    def centre(self, means):
        from . import _lib
        for t, mean in enumerate(means):
            self.ctx.ewise(_lib.OP_ADD, self.table.row(t), -float(mean))

    def gram(self):
        T = self.shape[0]
        return self.ctx.gemm(self.table, self.table, tb=True, out=np.empty((T, T)))


def correlation_of_rows_sharded(table, allreduce_sum):
    """Pearson correlation between the rows of the T x n table whose columns are spread over the ranks; `table` is this
    rank's columns (a HostTable / DeviceTable, centred in place), `allreduce_sum` sums a float64 array over the ranks
    in rank order.  Two passes, so that nothing cancels: global means from the all-reduced row sums and cell count,
    then the all-reduced Gram of the centred rows, normalised by the square roots of its diagonal.  Every rank makes
    the same two collective calls and ends with the same bits."""
    T, n_local = table.shape
    sums = allreduce_sum(np.concatenate([np.asarray(table.row_sums(), dtype=np.float64), [float(n_local)]]))
    table.centre(sums[:T] / sums[T])
    gram = np.asarray(allreduce_sum(np.asarray(table.gram(), dtype=np.float64).reshape(-1))).reshape(T, T)
    scale = np.sqrt(np.diag(gram))
    return gram / np.outer(scale, scale)


class TimePointEstimator(DensityEstimator):
    """DensityEstimator for one rank's slice of a gathered time point that decides what one rank would decide from all
    n_t cells: n_landmarks, gp_type and the parameter checks see n_t, the landmarks are clustered from the gathered
    cells (already the base class's rule under ranks), and the non-sparse GP -- which the library does not shard -- is
    fitted as what it is: the replicated factor Lp = chol(K(x_t, x_t) + jitter I) with this rank's rows of it as L, and
    a predictor with the gathered cells as centres.  x_t: the time point's cells in global order; lo: the global index
    of this rank's first cell among them."""

    def __init__(self, n_t, x_t, lo, **kwargs):
        super().__init__(**kwargs)
        self._time_point = (int(n_t), x_t, int(lo))
        self._x_all = (x_t, int(lo))      # what _all_cells() would gather from the ranks' slices

    def _compute_n_landmarks(self):
        return compute_n_landmarks(self.gp_type, self._time_point[0], self.landmarks)

    def _compute_gp_type(self):
        return compute_gp_type(self.n_landmarks, self.rank, self._time_point[0])

    def validate_parameter(self):
        validate_params(self.rank, self.gp_type, self._time_point[0], self.n_landmarks, self.landmarks)

    def _n_obs(self):
        return self._time_point[0]

    def _replicated_full(self):
        return self.gp_type == GaussianProcessType.FULL and self.landmarks is None and self.L is None

    def _device_fit(self):
        if self._fit is None and self._replicated_full():
            from . import _lib
            _, x_t, lo = self._time_point
            ctx = _lib.default_context()
            Lp = np.asarray(self.Lp, dtype=np.float64) if self.Lp is not None else \
                ctx.chol_lower(self.cov_func(x_t, x_t), add_diag=self.jitter, jitter=self.jitter)
            self._fit = _lib.Fit.from_L(ctx, np.ascontiguousarray(Lp[lo:lo + self.x.shape[0]]), Lp=Lp)
        return super()._device_fit()

    def _build_conditional(self):
        if not (self.gp_type == GaussianProcessType.FULL and self.landmarks is None):
            return super()._build_conditional()
        from .inference import compute_conditional
        return compute_conditional(self.x, self._time_point[1], self.pre_transformation, self.pre_transformation_std,
                                   self.log_density_x, self.mu, self.cov_func, self.L, self.Lp, sigma=None,
                                   jitter=self.jitter, y_is_mean=True,
                                   with_uncertainty=self.predictor_with_uncertainty)


def compute_ls_time_sharded(nn_distances, x, cov_func_curry, comm, times=None, warn_below=SMALL_TIME_POINT,
                            return_data=False, density_estimator_kwargs=None):
    """compute_ls_time when x / nn_distances are this rank's contiguous block of the cells (`comm`: the ranks'
    distributed.ShardedCommunicator).  The same value on every rank, bit for bit.  With `return_data` the tuple
    (ls_time, densities, estimators, time points): `densities` is T x n_local -- every time point's density on THIS
    rank's cells --, the estimators are the per-time-point fits (their predictors are replicated, their cells are this
    rank's slice of the re-sharded time point), the time points are the global ones."""
    from . import _lib
    xt = np.asarray(validate_time_x(x, times), dtype=np.float64)
    states, stamp = np.ascontiguousarray(xt[:, :-1]), xt[:, -1]
    nn_distances = np.asarray(nn_distances, dtype=np.float64)
    kwargs = dict(density_estimator_kwargs or {})
    stamps = global_time_points(comm.host, stamp)
    fitted = []
    for k, t in enumerate(stamps, start=1):
        x_t, nn_t = gather_time_point(comm.host, states, stamp, nn_distances, t)
        n_t = x_t.shape[0]
        if comm.rank == 0:
            logger.info(f"[{k} of {len(stamps)}] Computing density for {n_t:,} cells at time point {t}.")
            if n_t < warn_below:
                logger.warning(f"Time point {t} only has {n_t:,} cells. "
                               "This could lead to inaccurate estimation of the time length scale `ls_time`.")
        lo, hi = reshard_bounds(n_t, comm.world_size, comm.rank, t)
        model = TimePointEstimator(n_t, x_t, lo, nn_distances=nn_t[lo:hi], **kwargs)
        model.fit(np.ascontiguousarray(x_t[lo:hi]))
        fitted.append(model)
    # every time point's density on this rank's cells of all time points: T fused predict passes into one table in HBM
    ctx = _lib.default_context()
    T, n_local = len(fitted), states.shape[0]
    if n_local == 0:      # a rank without cells still takes part in both all-reduces
        densities = np.zeros((T, 0))
        target = correlation_of_rows_sharded(HostTable(np.zeros((T, 0))), ctx.allreduce_sum)
    else:
        cells, table = ctx.to_device(states), ctx.empty((T, n_local))
        try:
            for k, model in enumerate(fitted):
                model.predict.mean(cells, out=table.row(k))
            densities = table.to_host() if return_data else None      # (before the rows are centred in place)
            target = correlation_of_rows_sharded(DeviceTable(ctx, table), ctx.allreduce_sum)
        finally:
            table.free()
            cells.free()
    ls_time = float(comm.broadcast(_closest_length_scale(cov_func_curry, stamps, target), src=0))
    if return_data:
        return ls_time, densities, fitted, stamps
    return ls_time
