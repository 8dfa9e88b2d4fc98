"""DimensionalityEstimator (mellon/dimensionality_estimator.py): same constructor, attributes and
prepare_inference / run_inference / process_inference / fit / fit_predict flow, `predict` (local dimensionality) and
`predict_density`.  The k-NN search, the local fractal dimension, the covariance factorisation and the MAP objective of
the (log-dimensionality, log-density) pair run on the MI355X; SciPy's L-BFGS-B drives the objective from the host.
optimizer="advi" fits a mean-field Gaussian over both latent functions (inference.run_advi on the batched objective,
mln_dim_objective_batch); `pre_transformation_std` is then (2, m), one row per predictor.

Deliberate deviation: duplicate cells give a zero nearest-neighbour distance and log 0 in the likelihood; the reference's
solve then sees an infinite loss and stops where it started.  This estimator raises a ValueError naming the count of
zero distances (or of non-finite local dimensions) before the solve instead.

Cells sharded over the ranks of a communicator (distributed.current(), contiguous shards in rank order): every rank
searches ITS cells among the cells of ALL ranks (gathered once over the host communicator), so `distances`, `d`,
`nn_distances`, `local_dim_x` and `log_density_x` are this rank's rows of the single-rank arrays; the heuristics, the
landmarks, `Lp`, `pre_transformation` and both predictors are replicated.  Every decision (k, gp_type, n_landmarks, the
duplicate-cell errors) is taken on global counts, so all ranks raise -- or go on -- together."""
import logging

import numpy as np

from .base_model import BaseEstimator, DEFAULT_COV_FUNC
from .inference import (DEFAULT_INIT_LEARN_RATE, DEFAULT_JIT, DEFAULT_N_ITER, DEFAULT_OPTIMIZER,
                        compute_conditional, compute_conditional_explog, compute_dimensionality_loss_func,
                        compute_dimensionality_transform, compute_log_density_x)
from .parameter_validation import validate_params
from .parameters import (DEFAULT_RANDOM_SEED, compute_gp_type, compute_initial_dimensionalities, compute_mu,
                         compute_n_landmarks)
from .util import DEFAULT_JITTER, ensure_2d
from .validation import validate_array, validate_float, validate_k, validate_positive_int

logger = logging.getLogger("mellon")

LOCAL_DIM_K = 30      # neighbours of the local fractal dimension (util.local_dimensionality's default)
KNN_MAX_K = 64        # the device k-NN search's limit (mln_knn)


def _count_over_ranks(count):
    """A per-rank count of offending cells summed over the ranks: an error decided on the sum is raised by every rank
    (one raised by a single rank would leave the others waiting in the next collective).  Single rank: the count."""
    from .distributed import current
    return current().global_count(int(count))


class DimensionalityEstimator(BaseEstimator):
    """Local intrinsic dimensionality and density (reference dimensionality_estimator.py:35-677)."""

    def __init__(self, cov_func_curry=DEFAULT_COV_FUNC, n_landmarks=None, rank=None, gp_type=None,
                 jitter=DEFAULT_JITTER, optimizer=DEFAULT_OPTIMIZER, n_iter=DEFAULT_N_ITER,
                 init_learn_rate=DEFAULT_INIT_LEARN_RATE, landmarks=None, k=10, distances=None, d=None, mu_dim=0,
                 mu_dens=None, ls=None, ls_factor=1, cov_func=None, Lp=None, L=None, initial_value=None,
                 predictor_with_uncertainty=False, jit=DEFAULT_JIT, check_rank=None,
                 random_state=DEFAULT_RANDOM_SEED):
        super().__init__(cov_func_curry=cov_func_curry, n_landmarks=n_landmarks, rank=rank, gp_type=gp_type,
                         jitter=jitter, optimizer=optimizer, n_iter=n_iter, init_learn_rate=init_learn_rate,
                         landmarks=landmarks, nn_distances=None, d=d, mu=mu_dens, ls=ls, ls_factor=ls_factor,
                         cov_func=cov_func, Lp=Lp, L=L, initial_value=initial_value,
                         predictor_with_uncertainty=predictor_with_uncertainty, jit=jit, check_rank=check_rank,
                         random_state=random_state)
        self.k = validate_positive_int(k, "k")
        self.mu_dim = validate_float(mu_dim, "mu_dim")
        self.mu_dens = validate_float(mu_dens, "mu_dens", optional=True)
        self.distances = validate_array(distances, "distances", optional=True)
        self.transform = None
        self.loss_func = None
        self.opt_state = None
        self.losses = None
        self.pre_transformation = None
        self.pre_transformation_std = None
        self.local_dim_x = None
        self.log_density_x = None
        self.local_dim_func = None
        self.log_density_func = None

    def __repr__(self):
        def s(v):
            if v is None:
                return "None"
            return f"<array {tuple(v.shape)}>" if hasattr(v, "shape") else str(v)
        keys = ("n_landmarks", "rank", "gp_type", "jitter", "k", "d", "mu_dim", "mu_dens", "ls", "cov_func",
                "landmarks", "Lp", "L", "distances", "initial_value", "optimizer")
        return self.__class__.__name__ + "(" + ", ".join(f"{k}={s(getattr(self, k, None))}" for k in keys) + ")"

    # -- attribute computations (reference dimensionality_estimator.py:345-467) --------------------------------
    def _compute_distances(self):
        """The k nearest other cells (dimensionality_estimator.py:375-384).  While k + 1 <= 64 (the device search's
        limit), ONE exact device search with max(k + 1, 30) neighbours also gives the local dimension its neighbourhoods:
        column 0 is the cell itself (or a coincident cell, at distance 0), columns 1 .. k are the distances.  At k = 64
        the distances come from a search of k that skips the cell itself (the same multiset of distances), and the
        neighbourhoods from a search of their own."""
        if isinstance(self.k, (int, np.integer)) and self.k > KNN_MAX_K:
            raise ValueError(f"k={self.k}: the exact device k-NN search finds at most {KNN_MAX_K} neighbours per cell, "
                             f"so DimensionalityEstimator needs 1 <= k <= {KNN_MAX_K}.")
        logger.info("Computing distances.")
        from . import _lib
        # queries: this rank's cells; candidates: the cells of all ranks.  Indices are global (global_offset + local).
        x, y, lo = self._queries_and_candidates()
        n = x.shape[0] if y is None else y.shape[0]
        validate_k(self.k, n)              # against the GLOBAL count: a shard with fewer than k cells is legal
        ctx = _lib.default_context()
        kl = min(LOCAL_DIM_K, n)
        if self.k + 1 <= KNN_MAX_K:
            dist, idx = ctx.knn(x, max(self.k + 1, kl), y=y, return_index=True)
            self._knn_idx = (self.x, idx[:, :kl])
            return np.ascontiguousarray(dist[:, 1:self.k + 1])
        dist = ctx.knn(x, self.k, y=y, exclude_self=True, self_offset=lo, return_index=False)
        self._knn_idx = (self.x, ctx.knn(x, kl, y=y, return_index=True)[1])
        return np.ascontiguousarray(dist)

    def _queries_and_candidates(self):
        """(this rank's cells, the cells of all ranks, the global index of this rank's first cell); single rank:
        (x, None, 0) -- the search then runs on x against itself."""
        from .distributed import current
        x = self._host_x()
        if current().world_size == 1:
            return x, None, 0
        x_all, lo = self._all_cells()
        return x, np.ascontiguousarray(ensure_2d(x_all)), lo

    def _compute_nn_distances(self):
        nn = np.ascontiguousarray(np.asarray(self.distances, dtype=np.float64)[:, 0])
        zeros = _count_over_ranks(np.count_nonzero(nn <= 0))
        if zeros:
            raise ValueError(f"{zeros} cells have a nearest-neighbour distance of 0 (duplicate cells): the likelihood "
                             "takes its logarithm. Remove or jitter the duplicates.")
        return nn

    def _compute_d(self):
        from .util import local_dimensionality
        held = self.__dict__.pop("_knn_idx", None)
        x, y, _ = self._queries_and_candidates()
        if held is not None and held[0] is self.x:
            # the neighbourhoods hold global indices: rows of the cells of all ranks
            d = local_dimensionality(x if y is None else y, k=held[1].shape[1], neighbor_idx=held[1])
        elif y is None:
            d = local_dimensionality(x)
        else:
            d = local_dimensionality(y, x_query=x)
        bad = _count_over_ranks(np.count_nonzero(~np.isfinite(d)))
        if bad:
            raise ValueError(f"{bad} cells have a non-finite local dimension (a zero distance among their "
                             f"{LOCAL_DIM_K} nearest neighbours: duplicate cells). Remove or jitter the duplicates.")
        return d

    # decisions on the cells of ALL ranks: a small shard must not pick a gp type (or a landmark count) of its own
    def _compute_n_landmarks(self):
        return compute_n_landmarks(self.gp_type, self._n_cells_global(), self.landmarks)

    def _compute_gp_type(self):
        return compute_gp_type(self.n_landmarks, self.rank, self._n_cells_global())

    def validate_parameter(self):
        validate_params(self.rank, self.gp_type, self._n_cells_global(), self.n_landmarks, self.landmarks)

    def _compute_mu_dens(self):
        return compute_mu(self.nn_distances, self.d)

    def _compute_initial_value(self):
        return compute_initial_dimensionalities(self.x, self.mu_dim, self.mu_dens, self.L, self.nn_distances, self.d)

    def _compute_transform(self):
        return compute_dimensionality_transform(self.mu_dim, self.mu_dens, self.L)

    def _compute_loss_func(self):
        return compute_dimensionality_loss_func(self.distances, self.transform, self.initial_value.shape[0])

    def _host_x(self):
        from . import _lib
        x = self.x.to_host() if isinstance(self.x, _lib.DeviceArray) else self.x
        return np.ascontiguousarray(ensure_2d(np.asarray(x, dtype=np.float64)))

    def _set_local_dim_x(self):
        self.local_dim_x, self.log_density_x = compute_log_density_x(self.pre_transformation, self.transform)

    def _row(self, a, i):
        return None if a is None else np.asarray(a).reshape(2, -1)[i, :]

    def _set_local_dim_func(self):
        logger.info("Computing predictive dimensionality function.")
        self.local_dim_func = compute_conditional_explog(
            self.x, self.landmarks, self._row(self.pre_transformation, 0), self._row(self.pre_transformation_std, 0),
            self.local_dim_x, self.mu_dim, self.cov_func, self.L, self.Lp, sigma=None, jitter=self.jitter,
            y_is_mean=True, with_uncertainty=self.predictor_with_uncertainty)

    def _set_log_density_func(self):
        logger.info("Computing predictive density function.")
        self.log_density_func = compute_conditional(
            self.x, self.landmarks, self._row(self.pre_transformation, 1), self._row(self.pre_transformation_std, 1),
            self.log_density_x, self.mu_dens, self.cov_func, self.L, self.Lp, sigma=None, jitter=self.jitter,
            y_is_mean=True, with_uncertainty=self.predictor_with_uncertainty)

    # -- public flow (reference dimensionality_estimator.py:469-677) -----------------------------------------------
    _PIPELINE = ("n_landmarks", "rank", "gp_type", None, "distances", "nn_distances", "d", "mu_dens", "ls", "cov_func",
                 "landmarks", "Lp", "L", "initial_value", "transform", "loss_func")

    def prepare_inference(self, x):
        if x is None:
            if self.x is None:
                raise ValueError("Required argument x is missing and self.x has not been set.")
            x = self.x
        elif self.x is not None and self.x is not x:
            raise ValueError("self.x has been set already, but is not equal to the argument x.")
        self.set_x(x)
        from .util import log_nn_new_fit
        log_nn_new_fit()
        try:
            for attr in self._PIPELINE:
                if attr is None:
                    self.validate_parameter()
                else:
                    self._prepare_attribute(attr)
        finally:
            self._release_x_on_device()
        return self.loss_func, self.initial_value

    def run_inference(self, loss_func=None, initial_value=None, optimizer=None):
        if optimizer == "advi" and self.optimizer != "advi":
            # the one remaining limit: a prepared estimator is not switched to ADVI here (everything below serves it)
            raise NotImplementedError('run_inference does not switch a prepared DimensionalityEstimator to "advi": '
                                      'construct the estimator with optimizer="advi".')
        if loss_func is not None:
            self.loss_func = loss_func
        if initial_value is not None:
            self.initial_value = initial_value
        if optimizer is not None:
            self.optimizer = optimizer
        self._run_inference()
        self.pre_transformation = np.asarray(self.pre_transformation).reshape(2, -1)
        if self.pre_transformation_std is not None:
            self.pre_transformation_std = np.asarray(self.pre_transformation_std).reshape(2, -1)
        return self.pre_transformation

    def process_inference(self, pre_transformation=None, build_predict=True):
        if pre_transformation is not None:
            self.pre_transformation = validate_array(pre_transformation, "pre_transformation")
        self._set_local_dim_x()
        if build_predict:
            self._set_local_dim_func()
            self._set_log_density_func()
        return self.local_dim_x, self.log_density_x

    def fit(self, x=None, build_predict=True):
        self.prepare_inference(x)
        self.run_inference()
        self.process_inference(build_predict=build_predict)
        return self

    @property
    def predict_density(self):
        if self.log_density_func is None:
            self._set_log_density_func()
        return self.log_density_func

    @property
    def predict(self):
        if self.local_dim_func is None:
            self._set_local_dim_func()
        return self.local_dim_func

    def fit_predict(self, x=None, build_predict=False):
        if self.x is not None and x is not None and self.x is not x:
            raise ValueError("self.x has been set already, but is not equal to the argument x.")
        if self.x is None and x is None:
            raise ValueError("Required argument x is missing and self.x has not been set.")
        if x is None:
            x = self.x
        else:
            x = validate_array(x, "x")
        self.fit(x, build_predict=build_predict)
        return self.local_dim_x
