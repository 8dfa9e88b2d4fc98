"""mln_slogdet_batched: sign and log|det| of batches of small matrices, one wavefront per matrix, against an LU in
np.longdouble (tests/slogdet_reference.py).

Bound on logabsdet, per batch:  err_device <= 4 max_batch(err_LAPACK) + k^2 2^-52, both errors against the longdouble value
over the same batch.  The factor 4 allows a different but equally valid pivot / summation order; the floor is one rounding per
update of each of the k pivots.  Signs equal numpy's on every nonsingular matrix; exactly singular matrices give (0, -inf)."""
import numpy as np
import pytest

import slogdet_reference as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from mellon_amd import _lib
    return _lib.default_context()


def test_the_entry_exists(ctx):
    assert hasattr(ctx.lib, "mln_slogdet_batched")


@pytest.mark.parametrize("k", [1, 2, 3, 8, 31, 64])
def test_crafted_batches(ctx, k):
    for name, (A, singular) in sr.crafted(k).items():
        sign, logabs = ctx.slogdet_batched(A)
        assert sign.shape == logabs.shape == (A.shape[0],)
        if singular:
            assert np.array_equal(sign, np.zeros(A.shape[0])) and np.all(logabs == -np.inf), name
            continue
        assert np.linalg.cond(A).max() <= sr.COND_MAX or name == "odd permutation", name
        s_np, _ = np.linalg.slogdet(A)
        assert np.array_equal(sign, s_np), name
        assert np.array_equal(sign, sr.slogdet_longdouble(A)[0]), name
        e_dev, e_lap, bound = sr.logdet_errors(A, logabs)
        print(f"k = {k:2d} {name}: device {e_dev:.2e}, LAPACK {e_lap:.2e}, bound {bound:.2e}")
        assert e_dev <= bound, name
        s2, l2 = ctx.slogdet_batched(A)
        assert np.array_equal(s2, sign) and np.array_equal(l2, logabs), name       # two calls, identical bits


@pytest.mark.parametrize("k,lead", [(3, 1), (8, 5), (31, 30), (64, 63)])
def test_a_leading_block_of_padded_matrices(ctx, k, lead):
    """lead < k on a batch with lda > k k, through the C entry: the rows and columns beyond `lead` and the padding between
    the matrices (NaN here) are never read."""
    A = sr.crafted(k)["gaussian"][0]
    B, lda = A.shape[0], k * k + 7
    buf = np.full((B, lda), np.nan)
    buf[:, :k * k] = A.reshape(B, -1)
    sign, logabs = np.empty(B), np.empty(B)
    rc = ctx.lib.mln_slogdet_batched(ctx.handle, buf.ctypes.data, B, k, lda, lead, sign.ctypes.data, logabs.ctypes.data)
    assert rc == 0
    sub = np.ascontiguousarray(A[:, :lead, :lead])
    ok = np.linalg.cond(sub) <= sr.COND_MAX          # a leading block of a well-conditioned matrix need not be one
    assert ok.sum() >= B // 2
    assert np.array_equal(sign, np.linalg.slogdet(sub)[0])
    e_dev, e_lap, bound = sr.logdet_errors(sub[ok], logabs[ok])
    print(f"k = {k}, lead = {lead}: device {e_dev:.2e}, LAPACK {e_lap:.2e}, bound {bound:.2e}")
    assert e_dev <= bound
    s2, l2 = ctx.slogdet_batched(A, lead=lead)
    assert np.array_equal(s2, sign) and np.array_equal(l2, logabs)


def test_device_pointers_and_batch_shapes(ctx):
    A = sr.crafted(8)["symmetric indefinite"][0][:24]
    sign, logabs = ctx.slogdet_batched(A)
    s4, l4 = ctx.slogdet_batched(A.reshape(2, 3, 4, 8, 8))
    assert s4.shape == (2, 3, 4) and np.array_equal(s4.reshape(-1), sign) and np.array_equal(l4.reshape(-1), logabs)
    a_dev, s_dev, l_dev = ctx.to_device(A), ctx.to_device(np.zeros(24)), ctx.to_device(np.zeros(24))
    assert ctx.lib.mln_slogdet_batched(ctx.handle, a_dev.ptr, 24, 8, 64, 8, s_dev.ptr, l_dev.ptr) == 0
    assert np.array_equal(s_dev.to_host(), sign) and np.array_equal(l_dev.to_host(), logabs)
    for a in (a_dev, s_dev, l_dev):
        a.free()
    assert ctx.slogdet_batched(np.zeros((0, 3, 3)))[0].shape == (0,)


def test_what_the_device_does_not_factor_is_refused(ctx):
    with pytest.raises(NotImplementedError):
        ctx.slogdet_batched(np.tile(np.eye(65), (2, 1, 1)))                   # lead = 65
    sign, logabs = ctx.slogdet_batched(np.tile(np.eye(65), (2, 1, 1)), lead=64)
    assert np.array_equal(sign, np.ones(2)) and np.array_equal(logabs, np.zeros(2))
    with pytest.raises(Exception):
        ctx.slogdet_batched(np.eye(3)[None], lead=4)                          # lead > k
    with pytest.raises(Exception):
        ctx.slogdet_batched(np.eye(3)[None], lead=0)
    with pytest.raises(ValueError):
        ctx.slogdet_batched(np.zeros((2, 3, 4)))
