"""Sparse inputs at the door (no GPU): validate_array densifies anything sparse as the reference does, and the targets
validator turns a 2-D sparse y into the canonical CSR holder that mln_sparse_solve_csr reads."""
import numpy as np
import pytest
import scipy.sparse as sp

from mellon_amd.validation import CSRTargets, csr_targets, validate_array, validate_targets

FORMATS = [sp.csr_matrix, sp.csc_matrix, sp.coo_matrix, sp.csr_array, sp.csc_array, sp.coo_array]


def dense_example():
    rng = np.random.default_rng(0)
    A = rng.normal(size=(7, 5)) * (rng.random((7, 5)) < 0.4)
    A[2] = 0.0          # an empty row
    A[:, 3] = 0.0       # an empty column
    return A


def holder_equals(h, dense):
    """The holder is canonical CSR of `dense`'s shape and holds its values."""
    n, p = dense.shape
    assert isinstance(h, CSRTargets) and h.shape == (n, p) and h.ndim == 2
    assert h.indptr.dtype == np.int64 and h.indptr.shape == (n + 1,) and h.indptr[0] == 0 and h.indptr[-1] == h.nnz
    assert h.indices.dtype == np.int32 and h.data.dtype == np.float64 and h.indices.shape == h.data.shape
    for i in range(n):
        cols = h.indices[h.indptr[i]:h.indptr[i + 1]]
        assert np.all(np.diff(cols) > 0) and np.all((cols >= 0) & (cols < p))
    assert np.array_equal(h.toarray(), dense)
    assert np.array_equal(h.rows(1, n - 1), dense[1:n - 1])


@pytest.mark.parametrize("fmt", FORMATS)
def test_validate_array_densifies_sparse(fmt):
    A = dense_example()
    out = validate_array(fmt(A), "x", ndim=2)
    assert isinstance(out, np.ndarray) and type(out) is np.ndarray and out.dtype == np.float64
    assert np.array_equal(out, np.asarray(fmt(A).todense()))
    with pytest.raises(ValueError, match="dimensional"):
        validate_array(fmt(A), "x", ndim=1)
    assert np.array_equal(validate_array(fmt(A.astype(np.int32)), "x"), A.astype(np.int32).astype(np.float64))


def test_validate_array_dense_path_unchanged():
    A = dense_example()
    assert validate_array(A, "x") is A                       # identity (set_x relies on it)
    assert validate_array(A.astype(np.float32), "x").dtype == np.float64
    assert validate_array(None, "x", optional=True) is None
    with pytest.raises(TypeError):
        validate_array(None, "x")
    with pytest.raises(TypeError):
        validate_array(object(), "x")
    with pytest.raises(TypeError):
        validate_array(lambda: 0, "x")


def test_targets_validator_keeps_dense_and_1d():
    A = dense_example()
    assert validate_targets(A, "y") is A
    y1 = A[:, 0].copy()
    assert validate_targets(y1, "y") is y1
    t = validate_targets(A, "Y", transpose=True)
    assert isinstance(t, np.ndarray) and np.array_equal(t, A.T)
    with pytest.raises(TypeError):
        validate_targets(None, "y")


@pytest.mark.parametrize("fmt", FORMATS)
def test_holder_from_every_format(fmt):
    A = dense_example()
    holder_equals(validate_targets(fmt(A), "y"), A)


def test_holder_sorts_and_sums_duplicates():
    # row 0: columns given as 4, 1, 4 (a duplicate), row 1 empty, row 2: 3, 0
    indptr, indices = np.array([0, 3, 3, 5]), np.array([4, 1, 4, 3, 0])
    data = np.array([1.0, 2.0, 0.5, 4.0, 8.0])
    M = sp.csr_matrix((data, indices, indptr), shape=(3, 6))
    assert not M.has_canonical_format
    h = validate_targets(M, "y")
    assert np.array_equal(h.indptr, [0, 2, 2, 4]) and np.array_equal(h.indices, [1, 4, 0, 3])
    assert np.array_equal(h.data, [2.0, 1.5, 8.0, 4.0])
    assert np.array_equal(M.indices, [4, 1, 4, 3, 0])         # the caller's matrix is left as it was
    coo = sp.coo_matrix((np.array([1.0, 2.0, 4.0]), (np.array([1, 1, 0]), np.array([2, 2, 5]))), shape=(2, 6))
    h = validate_targets(coo, "y")
    assert np.array_equal(h.indptr, [0, 1, 2]) and np.array_equal(h.indices, [5, 2]) and np.array_equal(h.data, [4.0, 3.0])


def test_holder_keeps_explicit_zeros():
    M = sp.csr_matrix((np.array([0.0, 3.0, 0.0]), np.array([1, 2, 0]), np.array([0, 2, 3])), shape=(2, 4))
    h = validate_targets(M, "y")
    assert h.nnz == 3 and np.array_equal(h.data, [0.0, 3.0, 0.0]) and np.array_equal(h.indices, [1, 2, 0])
    holder_equals(h, M.toarray())


def test_holder_empty_rows_columns_and_all_zero():
    A = np.zeros((5, 4))
    A[1, 2] = 1.5            # rows 0, 2, 3, 4 and columns 0, 1, 3 empty
    holder_equals(validate_targets(sp.csr_matrix(A), "y"), A)
    Z = sp.csr_matrix((5, 4))
    h = validate_targets(Z, "y")
    assert h.nnz == 0 and np.array_equal(h.indptr, np.zeros(6, dtype=np.int64))
    holder_equals(h, np.zeros((5, 4)))
    holder_equals(validate_targets(sp.csr_matrix((1, 1)), "y"), np.zeros((1, 1)))


@pytest.mark.parametrize("dtype", [np.float32, np.int32, np.int64, bool])
def test_holder_converts_value_dtypes(dtype):
    A = (np.abs(dense_example()) * 3).astype(dtype)
    M = sp.csr_matrix(A)
    assert M.dtype == np.dtype(dtype)
    holder_equals(validate_targets(M, "y"), A.astype(np.float64))


@pytest.mark.parametrize("idx_dtype", [np.int32, np.int64])
def test_holder_accepts_both_index_widths(idx_dtype):
    A = dense_example()
    M = sp.csr_matrix(A)
    M.indices, M.indptr = M.indices.astype(idx_dtype), M.indptr.astype(idx_dtype)      # (the constructor would narrow them)
    assert M.indptr.dtype == M.indices.dtype == np.dtype(idx_dtype)
    holder_equals(validate_targets(M, "y"), A)


@pytest.mark.parametrize("fmt", [sp.csr_matrix, sp.csr_array, sp.csc_matrix, sp.coo_array])
def test_holder_of_the_transpose(fmt):
    """multi_fit_predict's layout: functions are ROWS of Y, the fit takes Y.T -- without a dense detour."""
    A = dense_example()                # (functions, cells)
    h = validate_targets(fmt(A), "Y", transpose=True)
    holder_equals(h, np.ascontiguousarray(A.T))
    g = csr_targets(sp.csr_matrix(np.ascontiguousarray(A.T)), "y")
    assert np.array_equal(h.indptr, g.indptr) and np.array_equal(h.indices, g.indices) and np.array_equal(h.data, g.data)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_holder_rejects_non_finite(bad):
    A = dense_example()
    A[4, 1] = bad
    with pytest.raises(ValueError, match="non-finite"):
        validate_targets(sp.csr_matrix(A), "y")


def test_holder_rejects_too_many_columns():
    M = sp.csr_matrix((np.array([1.0]), np.array([5], dtype=np.int64), np.array([0, 1], dtype=np.int64)), shape=(1, 2 ** 31))
    with pytest.raises(ValueError, match="2\\^31"):
        validate_targets(M, "y")


def test_sparse_1d_targets_are_densified():
    v = sp.coo_array(np.array([0.0, 2.0, 0.0, 1.0]))
    if v.ndim != 1:
        pytest.skip("this SciPy has no 1-D sparse arrays")
    out = validate_targets(v, "y")
    assert isinstance(out, np.ndarray) and np.array_equal(out, [0.0, 2.0, 0.0, 1.0])


def test_panel_rows_mirror():
    from mellon_amd import _lib
    assert _lib.CSR_PANEL_BYTES <= 128 << 20
    src = open(_lib.os.path.join(_lib._HERE, "csrc", "sparse_targets.hip")).read()
    assert f"CSR_PANEL_BYTES = {_lib.CSR_PANEL_BYTES >> 20}ll << 20" in src          # the constant the kernel driver uses
    P = _lib.csr_panel_rows
    assert P(1) == _lib.CSR_PANEL_BYTES // 8 and P(2 ** 30) == 64
    for p in (3, 127, 4096, 16384, 70000):
        assert P(p) % 64 == 0 and P(p) >= 64 and (P(p) == 64 or P(p) * 8 * p <= _lib.CSR_PANEL_BYTES)


def test_validation_recognises_sparse_without_scipy():
    """Sparse containers are recognised by their methods: the validators never import SciPy."""
    import re
    from mellon_amd import validation
    assert not re.search(r"^\s*(import|from)\s+scipy\b", open(validation.__file__).read(), re.M)
