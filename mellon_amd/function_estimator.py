"""FunctionEstimator (mellon/function_estimator.py): GP regression of y (n x p) on x with
noise sigma; no optimiser, only the conditional (function_estimator.py:318-374).

Cells sharded over the ranks of a communicator (distributed.current(), contiguous shards in rank order): every rank
calls fit / fit_predict / multi_fit_predict with ITS rows of x and of y (dense, or CSR rows as they are; with one sigma
per cell, its entries of sigma).  `est.x` and `est.y` stay this rank's shard; `n_landmarks`, `gp_type`, `ls`, `cov_func`,
the landmarks and the fitted predictor (weights, `L`, `Cs`, `W`, `variance_weights`, `n_obs` = the global count) are
replicated: the same bits on every rank.  Every decision (n_landmarks, gp_type, the refusal of the full GP, the input
errors, empty shards) is taken on global counts over the host communicator BEFORE the first device collective, so all
ranks raise -- or go on -- together.  Only the landmark conditional shards: a resolved gp_type of "full" raises
NotImplementedError on every rank.

The fitted predictor under ranks: `predict(X)` / `mean`, `gradient`, `hessian`, `hessian_log_determinant`, `covariance`,
`mean_covariance`, `uncertainty`, `obs_variance(X)` and `to_json` read replicated state only -- any rank may call them
alone, with any X.  `leverage(X)` and `loo_residuals_squared(X, y)` are COLLECTIVE: the landmark leverage is defined
through B^T B with B = cov(X, x_u) over the queried points (conditional.py:660-685), so X is this rank's shard of one
global query set, every rank must call, and each rank gets its rows."""
import logging

import numpy as np

from .base_model import BaseEstimator, DEFAULT_COV_FUNC
from .inference import DEFAULT_INIT_LEARN_RATE, DEFAULT_N_ITER, DEFAULT_OPTIMIZER, compute_conditional
from .parameters import DEFAULT_RANDOM_SEED
from .distributed import current
from .util import DEFAULT_JITTER, GaussianProcessType
from .parameter_validation import validate_params
from .parameters import compute_gp_type, compute_n_landmarks
from .validation import (CSRTargets, validate_array, validate_bool, validate_float, validate_float_or_iterable_numerical,
                         validate_targets)

logger = logging.getLogger("mellon")


def _raise_on_all_ranks(counts, messages):
    """The outcome of the per-rank input checks, gathered over the host communicator: `counts` are the ranks' cell
    counts, `messages` their error texts (None: the shard is fine).  Every rank evaluates the same lists, so every
    rank raises the same ValueError -- one raised by the offending rank alone would leave the others waiting in the
    first collective of the fit."""
    if any(c == 0 for c in counts):
        empty = [r for r, c in enumerate(counts) if c == 0]
        raise ValueError(f"ranks {empty} hold no cells (cells per rank: {list(counts)}): every rank of a cell-sharded "
                         "FunctionEstimator fit needs at least one cell.")
    bad = [(r, m) for r, m in enumerate(messages) if m is not None]
    if bad:
        raise ValueError(f"{len(bad)} of {len(messages)} ranks refuse their shard of the input; rank {bad[0][0]}: "
                         f"{bad[0][1]}")


def _check_shard(y, n_cells, sigma, y_is_mean):
    """What the landmark conditional (and, for dense non-finite targets, nobody) would refuse about THIS rank's rows,
    as ValueErrors raised before any device call: only used when the cells are sharded, where the refusal has to be
    agreed on by all ranks first."""
    from .conditional import _is_per_feature_sigma
    if y.shape[0] != n_cells:
        raise ValueError(f"X.shape[0] = {n_cells:,} (n_samples) should equal y.shape[0] = {y.shape[0]:,}.")
    if not isinstance(y, CSRTargets) and not np.all(np.isfinite(y)):       # (a CSR holder was checked when it was built)
        raise ValueError("'y' holds non-finite values.")
    if y_is_mean or sigma is None:
        return
    sig = np.asarray(sigma, dtype=np.float64)
    if not np.all(sig > 0):
        raise ValueError("sigma must be positive for the landmark conditional.")
    if sig.ndim >= 1 and not _is_per_feature_sigma(sig, y) and (y.ndim != 1 or sig.shape != y.shape):
        raise ValueError(f"Unsupported sigma configuration: sigma of shape {sig.shape} goes with neither the "
                         f"{y.shape[0]:,} cells of this rank (1-D y) nor the outputs of y {tuple(y.shape)}.")


class FunctionEstimator(BaseEstimator):
    """reference function_estimator.py:28-615."""

    def __init__(self, cov_func_curry=DEFAULT_COV_FUNC, n_landmarks=None, gp_type=None, jitter=DEFAULT_JITTER,
                 optimizer=DEFAULT_OPTIMIZER, n_iter=DEFAULT_N_ITER, init_learn_rate=DEFAULT_INIT_LEARN_RATE,
                 landmarks=None, nn_distances=None, mu=0, ls=None, ls_factor=1, cov_func=None, sigma=0,
                 y_is_mean=False, predictor_with_uncertainty=False, obs_variance=False, jit=True,
                 random_state=DEFAULT_RANDOM_SEED):
        super().__init__(cov_func_curry=cov_func_curry, n_landmarks=n_landmarks, rank=1.0, jitter=jitter,
                         gp_type=gp_type, landmarks=landmarks, nn_distances=nn_distances, mu=mu, ls=ls,
                         ls_factor=ls_factor, cov_func=cov_func,
                         predictor_with_uncertainty=predictor_with_uncertainty, jit=jit, random_state=random_state)
        self.y_is_mean = validate_bool(y_is_mean, "y_is_mean")
        self.mu = validate_float(mu, "mu")
        self.sigma = validate_float_or_iterable_numerical(sigma, "sigma", positive=True)
        self.obs_variance = validate_bool(obs_variance, "obs_variance")
        if self.gp_type in (GaussianProcessType.FULL_NYSTROEM, GaussianProcessType.SPARSE_NYSTROEM):
            raise ValueError(f"gp_type={gp_type} but the Nyström rank reduction is not available for the "
                             "Function Estimator. Use gp_type='cholesky' or gp_type='full' instead.")
        self.conditional = None
        self.y = None

    def __call__(self, x=None, y=None):
        return self.fit_predict(x=x, y=y)

    def prepare_inference(self, x):
        """reference function_estimator.py:295-316."""
        self.set_x(x)
        from .util import log_nn_new_fit
        log_nn_new_fit()
        try:
            self._prepare_attribute("n_landmarks")
            self._prepare_attribute("gp_type")
            if self.gp_type == GaussianProcessType.FULL:      # (decided from the global count: all ranks raise)
                self._require_single_process("full Gaussian process of the FunctionEstimator")
            if self.ls is None and self.cov_func is None:
                self._prepare_attribute("nn_distances")
            self._prepare_attribute("ls")
            self._prepare_attribute("cov_func")
            self._prepare_attribute("landmarks")
        finally:
            self._release_x_on_device()      # the HBM copy the 1-NN search / k-means shared: the conditional never uses it

    # decisions on the cells of ALL ranks: a small shard must not pick a gp type (or a landmark count) of its own
    def _compute_n_landmarks(self):
        return compute_n_landmarks(self.gp_type, self._n_cells_global(), self.landmarks)

    def _compute_gp_type(self):
        return compute_gp_type(self.n_landmarks, self.rank, self._n_cells_global())

    def validate_parameter(self):
        validate_params(self.rank, self.gp_type, self._n_cells_global(), self.n_landmarks, self.landmarks)

    def _compute_ls(self):
        if self.cov_func is not None:
            return getattr(self.cov_func, "ls", 1.0)
        comm = current()
        if comm.world_size > 1:
            # the single-rank value bit for bit: ONE sum over the nn distances of all cells in rank order (the sum of
            # the ranks' partial sums, which BaseEstimator's global mean forms, rounds differently)
            from .util import log_nn
            a = log_nn(comm.allgather_rows(self.nn_distances))
            return float(np.exp(float(a.sum() / float(a.size)) + 3.0)) * self.ls_factor
        return super()._compute_ls()

    def compute_conditional(self, x=None, y=None, obs_variance=None):
        """reference function_estimator.py:318-374."""
        x = self.x if x is None else validate_array(x, "x")
        if x is None:
            raise ValueError("Required argument x is missing and self.x has not been set.")
        if y is None:
            raise ValueError("Required argument y is missing.")
        obs_variance = self.obs_variance if obs_variance is None else obs_variance
        if not isinstance(y, CSRTargets):
            y = validate_targets(y, "y")            # a 2-D sparse y stays sparse (CSR) down to the device
        if self.landmarks is None:      # (replicated, so the same decision on every rank; e.g. n_landmarks >= all cells)
            self._require_single_process("full Gaussian process of the FunctionEstimator")
        n_obs = self._n_cells_global() if x is self.x else current().global_count(x.shape[0])
        self.conditional = compute_conditional(
            x, self.landmarks, None, None, y, self.mu, self.cov_func, None, None, self.sigma, jitter=self.jitter,
            y_is_mean=self.y_is_mean, with_uncertainty=self.predictor_with_uncertainty, obs_variance=obs_variance)
        self.conditional.n_obs = n_obs      # the cells of all ranks (single rank: what the conditional set itself)
        return self.conditional

    def fit(self, x=None, y=None, obs_variance=None):
        return self._fit_targets(x, y, obs_variance)

    def _fit_targets(self, x, y, obs_variance=None, functions_in_rows=False):
        """fit(); with functions_in_rows `y` holds one function per ROW (multi_fit_predict) and is transposed by the
        validator -- a sparse one without a dense detour."""
        x = self.set_x(x)
        name = "Y" if functions_in_rows else "y"
        comm = current()
        if comm.world_size == 1:
            targets = validate_targets(y, name, transpose=functions_in_rows)
            if targets.shape[0] != x.shape[0]:
                raise ValueError(f"X.shape[0] = {x.shape[0]:,} (n_samples) should equal y.shape[0] = {targets.shape[0]:,}.")
        else:
            # errors that depend on this rank's rows are agreed on over the host communicator before anything else
            targets = message = None
            try:
                targets = validate_targets(y, name, transpose=functions_in_rows)
                _check_shard(targets, x.shape[0], self.sigma, self.y_is_mean)
            except (TypeError, ValueError) as e:
                message = str(e)
            outcome = comm.host.allgather((int(x.shape[0]), message))
            _raise_on_all_ranks([c for c, _ in outcome], [m for _, m in outcome])
        self.prepare_inference(x)
        self.compute_conditional(x, targets, obs_variance=obs_variance)
        # the validated array as before; of a sparse y the caller's own object (its transpose for functions in rows)
        self.y = (y.T if functions_in_rows else y) if isinstance(targets, CSRTargets) else targets
        return self

    @property
    def predict(self):
        if self.conditional is None:
            raise ValueError("The estimator has not been fitted: call fit(x, y) first.")
        return self.conditional

    def leverage(self, X=None):
        """Leverage with the fitted sigma, at the training cells by default (function_estimator.py:443-459).
        Collective under ranks: every rank calls, with its shard of one global query set (default: its cells), and
        gets its rows."""
        return self.predict.leverage(self.x if X is None else X)

    def loo_residuals_squared(self, X=None, y=None):
        """Squared leave-one-out residuals r^2 / (1 - h)^2; without arguments the values cached by an
        `obs_variance=True` fit (function_estimator.py:461-487).  Under ranks: this rank's rows; collective (every rank
        calls, X and y its shard of one global query set) whenever the leverage has to be computed, i.e. unless the
        cached values are returned."""
        if X is None and y is None:
            if hasattr(self.predict, "_corrected_r2"):
                return self.predict._corrected_r2
            X, y = self.x, self.y
        else:
            X = self.x if X is None else X
            y = self.y if y is None else y
        return self.predict.loo_residuals_squared(X, y)

    def get_obs_variance(self, X=None):
        """Smoothed observation variance of the fitted predictor (function_estimator.py:489-505)."""
        return self.predict.obs_variance(self.x if X is None else X)

    def fit_predict(self, x=None, y=None, Xnew=None):
        self.fit(x, y)
        return self.predict(self.x if Xnew is None else validate_array(Xnew, "Xnew"))

    def multi_fit_predict(self, x=None, Y=None, Xnew=None):
        """Functions stored as ROWS of Y (reference function_estimator.py multi_fit_predict)."""
        self._fit_targets(x, Y, functions_in_rows=True)
        return self.predict(self.x if Xnew is None else validate_array(Xnew, "Xnew")).T
