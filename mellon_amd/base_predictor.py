"""Predictor API (mellon/base_predictor.py): `mean` / `__call__` on the device, plus the
reference's JSON wire format for the predictor state (base_predictor.py:541-734) so that
predictors fitted here load in upstream Mellon and vice versa.  Covariance / gradient /
uncertainty methods are outside the accelerated path and raise."""
import bz2
import gzip
import json
import logging
import sys
from datetime import datetime
from importlib import import_module
from math import log

import numpy as np

from . import _lib
from .base_cov import Covariance
from .util import deserialize, ensure_2d, make_multi_time_argument, make_serializable
from .validation import validate_array, validate_bool, validate_time_x

logger = logging.getLogger("mellon")
_REF_MODULE = "mellon.conditional"


class Predictor:
    """Mean function of a conditioned GP: mean(x) = mu + K(x, centers) @ weights."""

    n_obs = None
    d = None
    d_method = None
    _center_name = "landmarks"

    def __init__(self, cov_func, centers, weights, mu, n_obs=None, jitter=None, sigma=None):
        self.cov_func = cov_func
        setattr(self, self._center_name, np.ascontiguousarray(ensure_2d(centers), dtype=np.float64))
        self.weights = np.ascontiguousarray(weights, dtype=np.float64)
        self.mu = float(mu)
        self.jitter = jitter
        self.sigma = sigma
        self.per_feature_sigma = False
        self.n_input_features = getattr(self, self._center_name).shape[1]
        self.n_obs = n_obs
        self._state_variables = {self._center_name, "weights", "mu", "jitter", "sigma", "per_feature_sigma"}

    @property
    def centers(self):
        return getattr(self, self._center_name)

    def __repr__(self):
        return (f'A predictor of class "{self.__class__.__name__}" with covariance function '
                f'"{self.cov_func}" and data:\n' +
                "\n".join(f"    {k}: {np.shape(getattr(self, k))}" for k in sorted(self._state_variables)))

    # -- evaluation (conditional.py:366-373,651-658,899-906 through base_predictor.py:180-257) ------
    def _mean(self, Xnew, out=None):
        ctx = _lib.default_context()
        return ctx.predict_mean(self.cov_func.lower(self.n_input_features), Xnew, self.centers,
                                self.weights, self.mu, out=out)

    def mean(self, x, normalize=False, out=None):
        """reference base_predictor.py:180-257.  `out` (beyond the reference's signature): a _lib.DeviceArray that
        receives the predictions in HBM -- with HBM-resident queries a batched predict then moves nothing over PCIe."""
        x = validate_array(x, "x")
        if not isinstance(x, _lib.DeviceArray):
            x = np.ascontiguousarray(ensure_2d(x), dtype=np.float64)
        normalize = validate_bool(normalize, "normalize")
        if x.shape[1] != self.n_input_features:
            raise ValueError(
                f"The predictor was trained on data with {self.n_input_features} features. "
                f"However, the provided input data has {x.shape[1]} features. "
                "Please ensure that the input data has the same number of features as the training data.")
        if normalize:
            if self.n_obs is None or self.n_obs == 0:
                raise ValueError("Cannot normalize without n_obs. Please set self.n_obs to the number "
                                 "of samples/cells trained on to enable normalization.")
            if out is not None:
                raise ValueError("normalize=True is not combined with a device-resident output")
            return self._mean(x) - log(self.n_obs)
        return self._mean(x, out=out)

    __call__ = mean

    def gradient(self, x, jit=True):
        """Gradient of the predicted mean at each row of x, shape == x.shape (base_predictor.py:490-505).
        The reference differentiates `_mean` with jax.jacrev; here the analytic kernel gradient is
        contracted with the weights on the device.  `jit` is accepted and ignored."""
        x = self._check_features(x)
        ctx, desc = _lib.default_context(), self.cov_func.lower(self.n_input_features)
        # p outputs: (n, p, d), the layout derivatives.gradient gives (derivatives.py:76-80), in one device call
        return ctx.predict_gradient(desc, x, self.centers, self.weights)

    # -- predictive uncertainty (base_predictor.py:330-428; conditional.py _covariance / _mean_covariance) --
    def _check_features(self, x):
        x = validate_array(x, "x")
        x = np.ascontiguousarray(ensure_2d(x), dtype=np.float64)
        if x.shape[1] != self.n_input_features:
            raise ValueError(
                f"The predictor was trained on data with {self.n_input_features} features. "
                f"However, the provided input data has {x.shape[1]} features. "
                "Please ensure that the input data has the same number of features as the training data.")
        return x

    def _has_per_feature_sigma(self):
        """Whether the predictor was fitted with a sigma per output (base_predictor.py:360-362)."""
        return bool(getattr(self, "per_feature_sigma", False))

    def covariance(self, x, diag=True, noise_free=False):
        """k(x,x) - A A^T with A = cov(x, centers) L^-T (variances when diag=True).  A predictor fitted with a
        per-feature sigma only has the noise-free covariance and asks for `noise_free=True`
        (base_predictor.py:364-420)."""
        if self._has_per_feature_sigma() and not noise_free:
            raise ValueError(
                "This predictor was fitted with per-feature sigma, so the "
                "covariance is noise-free (sigma=0) and does not include "
                "observation noise. Pass noise_free=True to acknowledge this "
                "and obtain the noise-free covariance, then account for "
                "observation noise separately (e.g., via obs_variance).")
        x = self._check_features(x)
        if not hasattr(self, "L") or self.L is None:
            raise ValueError("The predictor was computed without covariance. "
                             "Recompute setting `with_uncertainty=True.`")
        ctx = _lib.default_context()
        desc = self.cov_func.lower(self.n_input_features)
        cov = ctx.predict_covariance(desc, x, self.centers, np.asarray(self.L), diag=diag)
        Cs = getattr(self, "Cs", None)
        if Cs is not None:
            # noisy landmark conditional (conditional.py:707-716): + |Cs^-1 K_ux|^2, i.e. k - (k - |Cs^-1 K|^2)
            kss = self.cov_func.diag(x) if diag else self.cov_func(x, x)
            cov = cov + (kss - ctx.predict_covariance(desc, x, self.centers, np.asarray(Cs), diag=diag))
        return cov

    def mean_covariance(self, x, diag=True):
        """(K W)(K W)^T: uncertainty of the mean inherited from the parameter uncertainty W."""
        x = self._check_features(x)
        if not hasattr(self, "W") or self.W is None:
            raise ValueError(
                "The predictor was computed without uncertainty, e.g., using ADVI. "
                "Recompute setting `with_uncertainty=True.` and define `pre_transformation_std`"
                ", e.g., by using `optimizer='advi'`.")
        return _lib.default_context().predict_mean_covariance(self.cov_func.lower(self.n_input_features), x,
                                                              self.centers, np.asarray(self.W), diag=diag)

    def uncertainty(self, x, diag=True):
        """covariance + mean_covariance (base_predictor.py:390-428)."""
        return self.covariance(x, diag=diag) + self.mean_covariance(x, diag=diag)

    def hessian(self, x, jit=True):
        """Hessian of the predicted mean at each row of x, shape x.shape + (d,) (base_predictor.py:507-521).  The
        reference applies jacfwd(jacrev(.)); here the closed-form second derivatives of the kernels are contracted
        with the weights on the device.  `jit` is accepted and ignored."""
        x = self._check_features(x)
        ctx, desc = _lib.default_context(), self.cov_func.lower(self.n_input_features)
        # p outputs: (n, p, d, d), the layout derivatives.hessian gives (derivatives.py:114-117), in one device call
        return ctx.predict_hessian(desc, x, self.centers, self.weights)

    _LOGDET_MIN_PAIRS = 1 << 16      # n_new m from which the Hessians are factored on the device (the GEMM routes' threshold)

    def _device_hessian_logdet(self, x, lead):
        """(signs, log |det|) of the leading lead x lead blocks of the Hessians of `Predictor.hessian` at the validated
        rows x, from the fused device entry -- or None where the host path has to run: a tree that is not one device
        program, a block the device does not factor, fewer than _LOGDET_MIN_PAIRS pairs (there the host path keeps its
        bits)."""
        ctx, desc = _lib.default_context(), self.cov_func.lower(self.n_input_features)
        if (isinstance(desc, _lib.BlockEvaluatedCov) or not 1 <= lead <= ctx.SLOGDET_MAX_LEAD
                or x.shape[0] * self.centers.shape[0] < self._LOGDET_MIN_PAIRS):
            return None
        return ctx.predict_hessian_logdet(desc, x, self.centers, self.weights, lead=lead)

    def hessian_log_determinant(self, x, jit=True):
        """(signs, log |det|) of the Hessian at each row of x (base_predictor.py:523-539).  From 2^16 (query, centre) pairs
        on the Hessians are built and factored on the device and only the two results come back; a subclass with a
        `hessian` of its own (ExpPredictor) gets numpy's slogdet of that."""
        if type(self).hessian is Predictor.hessian:
            fused = self._device_hessian_logdet(self._check_features(x), self.n_input_features)
            if fused is not None:
                return fused
        sign, logdet = np.linalg.slogdet(self.hessian(x))
        return sign, logdet

    # -- leverage / observation variance (base_predictor.py:263-355) -------------------------------------------
    def leverage(self, x):
        """Hat-matrix diagonal h_i used by the HC3 correction r^2 / (1 - h)^2.  A predictor fitted on cells sharded
        across ranks: COLLECTIVE for the landmark conditionals -- the leverage is defined through B^T B, B = cov(x, x_u),
        over the queried points, so x is this rank's shard of one global query set, every rank must call, and each
        rank gets its rows.  (mean, gradient, hessian, covariance, mean_covariance, uncertainty, obs_variance and
        to_json read replicated state only: any rank may call them alone.)"""
        x = self._check_features(x)
        if not hasattr(self, "_leverage"):
            raise NotImplementedError(f"{self.__class__.__name__} has no leverage.")
        if self.sigma is None:
            raise ValueError("leverage needs the noise level `sigma` of the fit.")
        return self._leverage(x, self.sigma)

    def loo_residuals_squared(self, x, y):
        """Squared leave-one-out residuals through the leverage shortcut (base_predictor.py:290-324).  Collective under
        ranks, like `leverage`: x, y are this rank's shard of one global query set."""
        x = self._check_features(x)
        y = np.asarray(validate_array(y, "y"), dtype=np.float64)
        residual = y - self._mean(x)
        h = self.leverage(x)
        if residual.ndim > h.ndim:
            h = h[..., None]
        return residual ** 2 / (1 - h) ** 2

    def obs_variance(self, x):
        """Smoothed observation variance: a second GP on the HC3-corrected squared residuals."""
        x = self._check_features(x)
        if getattr(self, "variance_weights", None) is None:
            raise ValueError("The predictor was computed without obs_variance. "
                             "Recompute setting `obs_variance=True`.")
        ctx = _lib.default_context()
        return ctx.predict_mean(self.cov_func.lower(self.n_input_features), x, self.centers,
                                np.asarray(self.variance_weights), float(self.variance_mu))

    # -- serialization --------------------------------------------------------------------------------
    def _data_dict(self):
        return {k: getattr(self, k) for k in self._state_variables}

    def __getstate__(self):
        from . import __version__
        data = self._data_dict()
        data.update({"n_input_features": self.n_input_features, "n_obs": self.n_obs, "d": self.d,
                     "d_method": self.d_method, "_state_variables": self._state_variables})
        return {
            "data": {k: make_serializable(v) for k, v in data.items()},
            "cov_func": self.cov_func.__getstate__(),
            "metadata": {"classname": self.__class__.__name__, "module_name": _REF_MODULE,
                         "module_version": __version__, "serialization_date": datetime.now().isoformat(),
                         "python_version": sys.version},
        }

    def __setstate__(self, state):
        for name, value in state["data"].items():
            setattr(self, name, deserialize(value))
        # files written by mellon 1.3.1 carry neither `_state_variables` nor `n_obs` (tests/test_density_estimator.py:
        # 139-151): every other entry of "data" is then a state variable, and n_obs stays None (normalize=True raises)
        meta = {"n_input_features", "n_obs", "d", "d_method", "_state_variables"}
        self._state_variables = set(getattr(self, "_state_variables", None) or (set(state["data"]) - meta))
        self.cov_func = Covariance.from_dict(state["cov_func"])
        for k in (self._center_name, "weights", "L", "W"):
            if getattr(self, k, None) is not None:
                setattr(self, k, np.ascontiguousarray(getattr(self, k), dtype=np.float64))

    def copy(self):
        new = self.__class__.__new__(self.__class__)
        new.__setstate__(self.__getstate__())
        return new

    def to_dict(self):
        return self.__getstate__()

    def to_json(self, filename=None, compress=None):
        json_str = json.dumps(self.to_dict())
        if filename is None:
            return json_str
        if compress == "gzip":
            filename = filename if str(filename).endswith(".gz") else str(filename) + ".gz"
            with gzip.open(filename, "wt") as f:
                f.write(json_str)
        elif compress == "bz2":
            filename = filename if str(filename).endswith(".bz2") else str(filename) + ".bz2"
            with bz2.open(filename, "wt") as f:
                f.write(json_str)
        elif compress is None:
            with open(filename, "w") as f:
                f.write(json_str)
        else:
            raise ValueError(f'Unknown compression format {compress}.\nAvailabe formats are "gzip", "bz2" and None.')
        logger.info(f"Written predictor to {filename}.")

    @classmethod
    def from_dict(cls, data_dict):
        clsname = data_dict["metadata"]["classname"]
        from . import conditional
        Sub = getattr(conditional, clsname, None)
        if Sub is None:
            Sub = getattr(import_module(data_dict["metadata"]["module_name"]), clsname)
        inst = Sub.__new__(Sub)
        inst.__setstate__(data_dict)
        return inst

    @classmethod
    def from_json_str(cls, json_str):
        return cls.from_dict(json.loads(json_str))

    @classmethod
    def from_json(cls, filepath, compress=None):
        filename = str(filepath)
        if compress == "gzip" or filename.endswith(".gz"):
            opener = gzip.open
        elif compress == "bz2" or filename.endswith(".bz2"):
            opener = bz2.open
        else:
            opener = open
        with opener(filepath, "rt") as f:
            return cls.from_json_str(f.read())


class ExpPredictor(Predictor):
    """exp of the mean (reference base_predictor.py ExpPredictor)."""

    def mean(self, x, logscale=False):
        """exp(mean), or the mean itself with `logscale=True` (base_predictor.py:748-787)."""
        logscale = validate_bool(logscale, "logscale")
        log_value = Predictor.mean(self, x)
        return log_value if logscale else np.exp(log_value)

    __call__ = mean

    def gradient(self, x, jit=True):
        return np.exp(Predictor.mean(self, x))[..., None] * Predictor.gradient(self, x)

    def hessian(self, x, jit=True):
        """Hessian of exp(f): e^f (H_f + grad f grad f^T)."""
        g = Predictor.gradient(self, x)
        return np.exp(Predictor.mean(self, x))[..., None, None] * (Predictor.hessian(self, x) + g[..., :, None] * g[..., None, :])


class PredictorTime(Predictor):
    """Predictor whose last input column is time (reference base_predictor.py:872-948)."""

    @make_multi_time_argument
    def mean(self, Xnew, time=None, normalize=False):
        Xnew = validate_array(Xnew, "Xnew")
        if isinstance(Xnew, _lib.DeviceArray) and time is None:
            return Predictor.mean(self, Xnew, normalize=normalize)      # HBM-resident queries [state | time]: used in place
        Xnew = np.ascontiguousarray(ensure_2d(Xnew), dtype=np.float64)
        x = validate_time_x(Xnew, time, n_features=self.n_input_features, cast_scalar=True)
        return Predictor.mean(self, np.ascontiguousarray(x), normalize=normalize)

    __call__ = mean

    @make_multi_time_argument
    def gradient(self, x, time=None, jit=True):
        """Gradient with respect to the state columns at the given time(s) (base_predictor.py:1094-1124)."""
        return Predictor.gradient(self, self._with_time(x, time))[..., :-1]

    @make_multi_time_argument
    def hessian(self, x, time=None, jit=True):
        """Hessian with respect to the state columns at the given time(s) (base_predictor.py:1127-1159)."""
        return Predictor.hessian(self, self._with_time(x, time))[..., :-1, :-1]

    @make_multi_time_argument
    def hessian_log_determinant(self, x, time=None, jit=True):
        """base_predictor.py:1162-1194.  The state columns are the leading (d - 1) x (d - 1) block of the full Hessian."""
        x = self._with_time(x, time)
        fused = self._device_hessian_logdet(x, self.n_input_features - 1)
        if fused is not None:
            return fused
        sign, logdet = np.linalg.slogdet(Predictor.hessian(self, x)[..., :-1, :-1])
        return sign, logdet

    @make_multi_time_argument
    def time_derivative(self, x, time=None, jit=True):
        """Derivative with respect to time (base_predictor.py:1052-1091)."""
        return Predictor.gradient(self, self._with_time(x, time))[..., -1]

    # -- multi_time on a grid: all T times in one pass (util.make_multi_time_argument looks for `_grid_<method>`) ----------
    # For cov = k_state(x, c) k_time(t, s) (parameters.compute_cov_func) the state factor carries all of the n m d work and
    # is the same for every time; the time factor folds into the weights:
    #   mean[i, t]  = mu + sum_j k_state(x_i, c_j) E[j, t],   E[j, t] = w_j k_time(t, s_j)
    #   d/dt [i, t] =      sum_j k_state(x_i, c_j) D[j, t],   D[j, t] = w_j g(t, s_j) (t - s_j)
    #   grad_x[i, t] = the T-output gradient of the state kernel with weights E
    # -- one multi-output prediction of the state kernel (kernel-matrix chunks + a GEMM) instead of T fused predictions.
    _GRID_MIN_WORK = 1 << 16      # n_new m T below which the per-time loop runs: launch-bound either way

    def _grid_split(self, Xnew, times):
        """(state descriptor, time leaf, [Xnew | 0]), or None when the per-time loop has to run."""
        from .base_cov import split_state_time
        if isinstance(Xnew, _lib.DeviceArray) or self.weights.ndim != 1 or times.shape[0] < 2:
            return None
        split = split_state_time(self.cov_func, self.n_input_features)
        if split is None:
            return None
        Xq = self._with_time(Xnew, 0.0)            # the loop's own validation; the state factor never reads the time column
        if Xq.shape[0] * self.centers.shape[0] * times.shape[0] < self._GRID_MIN_WORK:
            return None
        return split[0], split[1], Xq

    def _grid_setup(self, Xnew, times, want_derivative=False):
        """(state descriptor, [Xnew | 0], E, D or None), or None when the per-time loop has to run."""
        split = self._grid_split(Xnew, times)
        if split is None:
            return None
        state, time_leaf, Xq = split
        s = np.ascontiguousarray(self.centers[:, -1:])
        K, g = _lib.default_context().leaf_factors(time_leaf, times.reshape(-1, 1), s)        # (T, m) each
        E = np.ascontiguousarray((K * self.weights).T)
        D = np.ascontiguousarray((g * (times[:, None] - s[:, 0]) * self.weights).T) if want_derivative else None
        return state, Xq, E, D

    def _grid_mean(self, Xnew, time=None, normalize=False, times=None):
        normalize = validate_bool(normalize, "normalize")
        if normalize and (self.n_obs is None or self.n_obs == 0):
            return NotImplemented                  # the loop raises the predictor's own error
        setup = self._grid_setup(validate_array(Xnew, "Xnew"), times)
        if setup is None:
            return NotImplemented
        state, Xq, E, _ = setup
        out = _lib.default_context().predict_mean(state, Xq, self.centers, E, self.mu)
        return out - log(self.n_obs) if normalize else out

    def _grid_gradient(self, x, time=None, jit=True, times=None):
        setup = self._grid_setup(x, times)
        if setup is None:
            return NotImplemented
        state, Xq, E, _ = setup
        return np.ascontiguousarray(_lib.default_context().predict_gradient(state, Xq, self.centers, E)[..., :-1])

    # hess_x[i, t] = the T-output Hessian of the state kernel with weights E, its leading (d - 1) x (d - 1) block.  The device
    # call returns (n, T_b, d, d) with the time row and column; times go in blocks of T_b so that one call's result stays
    # within _GRID_HESSIAN_DOUBLES, and each block's state columns are copied into the (n, T, d - 1, d - 1) result.
    _GRID_HESSIAN_DOUBLES = 1 << 28      # 2 GiB of host memory per device call

    def _grid_hessian(self, x, time=None, jit=True, times=None):
        setup = self._grid_setup(x, times)
        if setup is None:
            return NotImplemented
        state, Xq, E, _ = setup
        ctx = _lib.default_context()
        n, d = Xq.shape
        T = times.shape[0]
        tb = max(1, self._GRID_HESSIAN_DOUBLES // max(1, n * d * d))
        if tb >= T:
            return np.ascontiguousarray(ctx.predict_hessian(state, Xq, self.centers, E)[..., :-1, :-1])
        out = np.empty((n, T, d - 1, d - 1), dtype=np.float64)
        for t0 in range(0, T, tb):
            out[:, t0:t0 + tb] = ctx.predict_hessian(state, Xq, self.centers,
                                                     np.ascontiguousarray(E[:, t0:t0 + tb]))[..., :-1, :-1]
        return out

    def _grid_hessian_log_determinant(self, x, time=None, jit=True, times=None):
        lead = self.n_input_features - 1
        if not 1 <= lead <= _lib.Context.SLOGDET_MAX_LEAD:
            return NotImplemented                  # the loop's host path factors what the device does not
        setup = self._grid_setup(x, times)
        if setup is None:
            return NotImplemented
        state, Xq, E, _ = setup
        return _lib.default_context().predict_hessian_logdet(state, Xq, self.centers, E, lead=lead)

    def _grid_time_derivative(self, x, time=None, jit=True, times=None):
        setup = self._grid_setup(x, times, want_derivative=True)
        if setup is None:
            return NotImplemented
        state, Xq, _, D = setup
        return _lib.default_context().predict_mean(state, Xq, self.centers, D, 0.0)

    # The variances on a grid: the kernel row at time t is the state row scaled by S[t, j] = k_time(t, s_j), so
    # one device call evaluates the state rows once per row chunk, stacks the scaled rows of a block of times into one tall
    # panel and runs the triangular solve / the product with W once on it -- L, Cs and W go up once, not once per time.
    _GRID_VARIANCE_DOUBLES = 0           # scratch budget of that call in doubles (0: the library's default, 2^27)

    def _grid_std(self):
        """The std of W = L^-T diag(std) while L and W are the arrays _attach_uncertainty stored, else None."""
        rec = getattr(self, "_uncertainty_std", None)
        if rec is not None and rec[0] is getattr(self, "L", None) and rec[1] is getattr(self, "W", None):
            return rec[2]
        return None

    def _grid_variances(self, Xnew, times, diag, want):
        """The (n, T) arrays named by `want` ("cov", "mcov") from one device call, or NotImplemented when the per-time loop
        has to run: full matrices (diag=False), a missing factor (the loop raises the predictor's own error), or any of
        _grid_split's conditions."""
        if not diag or ("cov" in want and getattr(self, "L", None) is None) \
                or ("mcov" in want and getattr(self, "W", None) is None):
            return NotImplemented
        split = self._grid_split(Xnew, times)
        if split is None:
            return NotImplemented
        state, time_leaf, Xq = split
        ctx = _lib.default_context()
        tcol = np.ascontiguousarray(times.reshape(-1, 1))
        S, _ = ctx.leaf_factors(time_leaf, tcol, np.ascontiguousarray(self.centers[:, -1:]))      # (T, m)
        kdiag = np.ascontiguousarray(np.diagonal(ctx.leaf_factors(time_leaf, tcol, tcol)[0]))     # k_time(t, t)
        std = self._grid_std() if "mcov" in want else None
        return ctx.predict_variance_grid(
            state, Xq, self.centers, S, kdiag, None if getattr(self, "L", None) is None else np.asarray(self.L),
            Cs=getattr(self, "Cs", None) if "cov" in want else None,
            W=np.asarray(self.W) if "mcov" in want and std is None else None, std=std, want=want,
            scratch_doubles=self._GRID_VARIANCE_DOUBLES)

    def _grid_covariance(self, Xnew, time=None, diag=True, noise_free=False, times=None):
        if self._has_per_feature_sigma() and not noise_free:
            return NotImplemented                  # the loop raises the predictor's own error
        return self._grid_variances(Xnew, times, diag, ("cov",))

    def _grid_mean_covariance(self, Xnew, time=None, diag=True, times=None):
        return self._grid_variances(Xnew, times, diag, ("mcov",))

    def _grid_uncertainty(self, Xnew, time=None, diag=True, times=None):
        if self._has_per_feature_sigma():
            return NotImplemented
        out = self._grid_variances(Xnew, times, diag, ("cov", "mcov"))
        return out if out is NotImplemented else out[0] + out[1]

    def _with_time(self, Xnew, time):
        Xnew = np.ascontiguousarray(ensure_2d(validate_array(Xnew, "Xnew")), dtype=np.float64)
        return np.ascontiguousarray(validate_time_x(Xnew, time, n_features=self.n_input_features, cast_scalar=True))

    @make_multi_time_argument
    def covariance(self, Xnew, time=None, diag=True, noise_free=False):
        return Predictor.covariance(self, self._with_time(Xnew, time), diag=diag, noise_free=noise_free)

    @make_multi_time_argument
    def mean_covariance(self, Xnew, time=None, diag=True):
        return Predictor.mean_covariance(self, self._with_time(Xnew, time), diag=diag)

    @make_multi_time_argument
    def uncertainty(self, Xnew, time=None, diag=True):
        x = self._with_time(Xnew, time)
        return Predictor.covariance(self, x, diag=diag) + Predictor.mean_covariance(self, x, diag=diag)
