"""The predictor gradient and Hessian routes return the bits they returned before they were given one driver per derivative order.

tests/golden/deriv_routes_parent.npz records Context.predict_gradient, Context.predict_hessian and
Context.predict_hessian_logdet at commit c121d74 ("Batch Hessians over outputs and times; factor them on the device"), the last
one with a launcher per route, for the cases of tools/deriv_routes_dump.py: the smallest call, the per-column route, the GEMM
routes single-output and batched with ragged tiles, the row-chunk seams of both derivative orders, and the same with one output
per block.  Every output is recomputed here and compared with np.array_equal (which takes -0.0 for 0.0: the one difference a
gradient that is accumulated into a zeroed result instead of assigned may show).  A mismatch is a defect of the launchers, not
a matter of tolerance.

To re-record (only when a change of arithmetic is intended): on the GPU box, `python tools/deriv_routes_dump.py` at the commit
whose bits are to be kept, and commit the file it writes."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("deriv_routes_dump", os.path.join(ROOT, "tools", "deriv_routes_dump.py"))
dump = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dump)


@pytest.fixture(scope="module")
def ctx():
    from mellon_amd import _lib
    return _lib.default_context()


@pytest.fixture(scope="module")
def pinned():
    return dump.load()


def test_the_fixture_covers_every_case(pinned):
    assert {name.split("/")[0] for name in pinned} == set(dump.cases())
    assert os.path.getsize(dump.FIXTURE) < 256 * 1024


@pytest.mark.parametrize("key", list(dump.cases()))
def test_bits_of_the_recorded_commit(ctx, pinned, key):
    got = dump.outputs(ctx, key)
    assert set(got) == {name for name in pinned if name.split("/")[0] == key}
    for name, a in got.items():
        assert a.shape == pinned[name].shape, name
        assert np.array_equal(a, pinned[name]), name
