"""Input validators with the error behaviour of mellon/validation.py (TypeError for None /
non-array input, ValueError for shapes and ranges); arrays come back as float64 NumPy."""
import logging

import numpy as np

logger = logging.getLogger("mellon")


def _is_sparse(a):
    """A sparse container, by its methods (SciPy's *_matrix / *_array and anything shaped like them)."""
    return hasattr(a, "todense") or (hasattr(a, "toarray") and hasattr(a, "tocsr"))


class CSRTargets:
    """2-D targets (n x p) kept sparse on the host, in the layout mln_sparse_solve_csr reads: `indptr` int64 (n + 1),
    `indices` int32 (nnz), `data` float64 (nnz).  Canonical: per row the indices strictly increase (sorted, duplicates
    summed); stored zeros stay stored values."""
    ndim = 2

    def __init__(self, indptr, indices, data, shape):
        self.indptr, self.indices, self.data = indptr, indices, data
        self.shape = (int(shape[0]), int(shape[1]))

    @property
    def nnz(self):
        return int(self.data.shape[0])

    def rows(self, i0, i1):
        """Rows [i0, i1) as a dense float64 block."""
        i0, i1 = max(0, int(i0)), min(self.shape[0], int(i1))
        out = np.zeros((max(i1 - i0, 0), self.shape[1]), dtype=np.float64)
        if i1 > i0:
            q0, q1 = int(self.indptr[i0]), int(self.indptr[i1])
            r = np.repeat(np.arange(i1 - i0), np.diff(self.indptr[i0:i1 + 1]))
            out[r, self.indices[q0:q1]] = self.data[q0:q1]
        return out

    def toarray(self):
        return self.rows(0, self.shape[0])


def csr_targets(sparse, name, transpose=False):
    """The canonical CSRTargets of a 2-D sparse container (of its transpose with `transpose`: the rows-are-functions layout
    of multi_fit_predict), through the container's own `tocsr()`; no dense array is formed."""
    c = (sparse.T if transpose else sparse).tocsr()
    n, p = (int(s) for s in c.shape)
    if p >= 2 ** 31:
        raise ValueError(f"'{name}' has {p:,} columns; sparse targets take fewer than 2^31.")
    try:
        data = np.ascontiguousarray(c.data, dtype=np.float64)
    except (TypeError, ValueError):
        raise TypeError(f"'{name}' should be numeric, got sparse data of dtype {getattr(c.data, 'dtype', None)} instead.")
    indptr = np.ascontiguousarray(c.indptr, dtype=np.int64)
    cols = np.asarray(c.indices, dtype=np.int64)
    if indptr.shape != (n + 1,) or indptr[0] != 0 or indptr[-1] != data.shape[0] or cols.shape != data.shape \
            or np.any(np.diff(indptr) < 0) or (cols.size and (cols.min() < 0 or cols.max() >= p)):
        raise ValueError(f"'{name}' is not a valid CSR matrix (indptr / indices do not describe its shape {(n, p)}).")
    if not np.all(np.isfinite(data)):
        raise ValueError(f"'{name}' holds non-finite values.")
    # canonical form: position = row * p + column strictly increasing; otherwise sort and sum what shares a position
    key = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr)) * p + cols
    if key.size > 1 and not np.all(key[1:] > key[:-1]):
        order = np.argsort(key, kind="stable")
        key, data = key[order], data[order]
        first = np.flatnonzero(np.concatenate(([True], key[1:] != key[:-1])))
        key, data = key[first], np.add.reduceat(data, first)
        cols = key % p
        indptr = np.concatenate(([0], np.cumsum(np.bincount(key // p, minlength=n)))).astype(np.int64)
    # (float64 data in canonical order is used in place: the holder is read-only and lives for one fit)
    return CSRTargets(indptr, np.ascontiguousarray(cols, dtype=np.int32), np.ascontiguousarray(data), (n, p))


def validate_targets(y, name, transpose=False):
    """The targets of a FunctionEstimator fit: a 2-D sparse container stays sparse (CSRTargets), everything else is
    validate_array's dense float64 array (transposed with `transpose`)."""
    if y is not None and _is_sparse(y) and hasattr(y, "tocsr") and len(getattr(y, "shape", ())) == 2:
        return csr_targets(y, name, transpose=transpose)
    y = validate_array(y, name)
    return y.T if transpose else y


def dense_targets(y):
    """A dense float64 array of the targets, whatever validate_targets returned."""
    return y.toarray() if isinstance(y, CSRTargets) else y


def validate_array(iterable, name, optional=False, ndim=None):
    """reference validation.py:302-361."""
    if iterable is None:
        if optional:
            return None
        raise TypeError(f"'{name}' can't be None.")
    from ._lib import DeviceArray
    if isinstance(iterable, DeviceArray):
        return iterable
    if isinstance(iterable, np.ndarray) and iterable.dtype == np.float64:
        array = iterable      # identity is preserved on purpose (set_x compares with `is`)
    elif _is_sparse(iterable):
        # reference validation.py:344-345: anything with `todense` is densified (recognised by its methods: no SciPy import)
        dense = iterable.toarray() if hasattr(iterable, "toarray") else iterable.todense()
        array = np.ascontiguousarray(np.asarray(dense), dtype=np.float64)
    else:
        try:
            array = np.asarray(iterable, dtype=np.float64)
        except (TypeError, ValueError):
            raise TypeError(f"'{name}' should be iterable and numeric, got {type(iterable)} instead.")
    if array.ndim == 0 and not np.ndim(iterable) == 0:
        raise TypeError(f"'{name}' should be iterable, got {type(iterable)} instead.")
    if ndim is not None:
        dims = (ndim,) if isinstance(ndim, int) else tuple(ndim)
        if array.ndim not in dims:
            raise ValueError(f"'{name}' must be a {dims}-dimensional array, got {array.ndim}D array instead.")
    return array


def _is_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def validate_float_or_int(value, param_name, optional=False):
    """reference validation.py:104-150."""
    if value is None and optional:
        return None
    if isinstance(value, (int, np.integer)) and not isinstance(value, bool):
        return int(value)
    try:
        value = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"'{param_name}' should be a float or an int but is {type(value)}")
    if np.isnan(value):
        raise ValueError(f"'{param_name}' should be a non-NaN float number")
    return value


def validate_positive_float(value, param_name, optional=False):
    """reference validation.py:153-201."""
    if value is None and optional:
        return None
    try:
        value = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"'{param_name}' should be a float number but is {type(value)}")
    if value < 0:
        raise ValueError(f"'{param_name}' should be a positive float number")
    if np.isnan(value):
        raise ValueError(f"'{param_name}' should be a non-NaN float number")
    return value


def validate_float(value, param_name, optional=False):
    """reference validation.py:204-259."""
    if value is None:
        if optional:
            return None
        raise ValueError(f"'{param_name}' should be a float number but is None")
    try:
        value = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"'{param_name}' should be a float number but is {type(value)}")
    if np.isnan(value):
        raise ValueError(f"'{param_name}' should be a non-NaN float number")
    return value


def validate_positive_int(value, param_name, optional=False):
    """reference validation.py:262-299 (0 is accepted: n_landmarks=0 means 'full')."""
    if value is None and optional:
        return None
    ok = isinstance(value, (int, np.integer)) and not isinstance(value, bool)
    if not ok and isinstance(value, (float, np.floating)) and float(value).is_integer():
        ok, value = True, int(value)
    if not ok or value < 0:
        raise ValueError(f"'{param_name}' should be a positive integer number")
    return int(value)


def validate_bool(value, name, optional=False):
    """reference validation.py:364-400."""
    if value is None:
        if optional:
            return None
        raise TypeError(f"'{name}' can't be None.")
    if not isinstance(value, (bool, np.bool_)):
        raise TypeError(f"{name} should be of type bool, got {type(value)} instead.")
    return bool(value)


def validate_string(value, name, choices=None):
    """reference validation.py:403-435."""
    if not isinstance(value, str):
        raise TypeError(f"{name} should be of type str, got {type(value)} instead.")
    if choices is not None and value not in choices:
        raise ValueError(f"{name} should be one of {choices}, got '{value}' instead.")
    return value


def validate_float_or_iterable_numerical(value, name, optional=False, positive=False):
    """reference validation.py:438-494."""
    if value is None and optional:
        return None
    if _is_number(value):
        if positive and value < 0:
            raise ValueError(f"{name} should be a non-negative number or array")
        return float(value)
    if hasattr(value, "__iter__") or isinstance(value, np.ndarray):
        arr = np.asarray(value, dtype=np.float64)
        if positive and np.any(arr < 0):
            raise ValueError(f"All elements in {name} should be non-negative")
        return arr if arr.ndim > 0 else float(arr)
    raise TypeError(f"'{name}' should be a number or an iterable of numbers, got {type(value)} instead.")


def validate_1d(x):
    """reference validation.py:497-525."""
    x = np.asarray(x)
    if x.ndim == 0:
        x = x[None]
    if x.ndim != 1:
        raise ValueError("`x` must be exactly 1-dimensional.")
    return x


def validate_nn_distances(nn_distances, optional=False):
    """reference validation.py:528-592: NaN / inf / <= 0 are replaced by the smallest positive
    distance; if every entry is invalid a ValueError is raised."""
    if nn_distances is None:
        if optional:
            return None
        raise ValueError("nn_distances are required but None is given.")
    nn = np.asarray(nn_distances, dtype=np.float64)
    # the common case in two passes: smallest > 0 and largest finite (a NaN anywhere makes either comparison false)
    if nn.ndim == 1 and nn.size and nn.min() > 0 and nn.max() < np.inf:
        return nn
    bad = np.isnan(nn) | np.isinf(nn) | (nn <= 0)
    n_bad = int(bad.sum())
    if n_bad == nn.size:
        raise ValueError(
            f"All {n_bad:,} computed nearest neighbor distances (`nn_distances` attribute) contain invalid "
            "values. Please check the input data.")
    if n_bad:
        logger.warning(
            f"The computed nearest neighbor distances (`nn_distances` attribute) contain {n_bad:,} invalid "
            "values. Setting invalid distances to the minimum positive value found.")
        nn = np.where(~bad, nn, nn[~bad].min())
    return nn


def validate_nn_distances_sharded(nn_distances, comm):
    """validate_nn_distances for a cell-sharded fit: the replacement value is the smallest positive distance over
    the cells of ALL ranks (the reference sees all cells, validation.py:528-592), and "every entry invalid" is
    decided -- and raised -- on every rank together, so no rank walks into a collective alone."""
    if comm is None or comm.world_size == 1:
        return validate_nn_distances(nn_distances)
    nn = np.asarray(nn_distances, dtype=np.float64)
    bad = np.isnan(nn) | np.isinf(nn) | (nn <= 0)
    local_min = float(nn[~bad].min()) if (~bad).any() else np.inf
    stats = comm.host.allgather((local_min, int(bad.sum()), int(nn.size)))
    n_bad, n_all = sum(s[1] for s in stats), sum(s[2] for s in stats)
    if n_bad == n_all:
        raise ValueError(
            f"All {n_bad:,} computed nearest neighbor distances (`nn_distances` attribute) contain invalid "
            "values. Please check the input data.")
    if n_bad:
        if comm.rank == 0:
            logger.warning(
                f"The computed nearest neighbor distances (`nn_distances` attribute) contain {n_bad:,} invalid "
                "values. Setting invalid distances to the minimum positive value found.")
        nn = np.where(~bad, nn, min(s[0] for s in stats))
    return nn


def validate_k(k, n_samples):
    """reference validation.py:595-612."""
    if not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError(f"k={k} must be a positive integer.")
    if n_samples < 2:
        raise ValueError(f"At least two samples are required to compute nearest neighbors but got {n_samples}.")
    if k >= n_samples:
        raise ValueError(f"k={k} must be smaller than the number of samples {n_samples}.")


def validate_time_x(x, times=None, n_features=None, cast_scalar=False):
    """reference validation.py:23-102: append `times` as the last column of x."""
    x = validate_array(x, "x", ndim=2)
    if cast_scalar and times is not None and (np.isscalar(times) or all(s == 1 for s in np.shape(times))):
        times = np.full(x.shape[0], float(np.asarray(times).reshape(-1)[0]))
    times = validate_array(times, "times", optional=True, ndim=(1, 2))
    if times is not None:
        if times.ndim == 1:
            times = times.reshape(-1, 1)
        elif times.shape[1] != 1:
            raise ValueError("'times' must be a 1D array or a 2D array with 1 column.")
        if x.shape[0] != times.shape[0]:
            raise ValueError(
                "'x' and 'times' must have the same number of samples. "
                f"Got {x.shape[0]} for 'x' and {times.shape[0]} for 'times'.")
        x = np.concatenate((x, times), axis=1)
    if n_features is not None:
        if x.shape[1] == n_features - 1 and times is None:
            raise ValueError(
                f"Expected {n_features} features including 'times' in 'x' but "
                f"only found {x.shape[1]} features and 'times' is not provided.")
        if x.shape[1] != n_features:
            raise ValueError(f"Wrong number of features in 'x'. Expected {n_features} but got {x.shape[1]}.")
    return x
