"""ctx.kmeans bit for bit against the build before the level driver of csrc/kmeans.hip was split into stages: one case per path
through the old function (tools/kmeans_pins.py lists them and wrote tests/golden/kmeans_pins.json with that build, twice, to
the same bytes -- the cluster sums are fixed-point and the seeding draws from block sums).  The other k-means tests compare a
build with itself; this one notices a launch that moved, a draw that went missing or a predicate that changed."""
import importlib.util
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("kmeans_pins", os.path.join(ROOT, "tools", "kmeans_pins.py"))
pins = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pins)

with open(os.path.join(ROOT, "tests", "golden", "kmeans_pins.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def ctx():
    from mellon_amd import _lib
    return _lib.default_context()


def test_every_case_is_pinned():
    assert sorted(GOLDEN) == sorted(pins.CASES)


@pytest.mark.parametrize("name", list(pins.CASES))
def test_kmeans_matches_the_pinned_bits(ctx, name):
    assert pins.run_case(ctx, name) == GOLDEN[name]


def test_kmeans_refuses_non_finite_cells(ctx, monkeypatch):
    from mellon_amd._lib import MellonHipError
    x = pins.case_input("mfma")
    x[1234, 5] = np.nan
    monkeypatch.setenv("MELLON_AMD_KM_LEVELS", "1")
    with pytest.raises(MellonHipError, match="non-finite"):
        ctx.kmeans(x, pins.CASES["mfma"][2])
