"""Cells with 65 to 256 features, the parts that need no GPU: where the landmarks are computed by default, and the two
diagnostics of the wide row-minimum sweep in the header and the binding."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("d,want", [(100, "hip"), (256, "hip"), (257, "sklearn"), (65, "hip"), (64, "hip"), (50, "hip"), (1, "hip")])
def test_landmarks_backend_feature_range(d, want):
    from mellon_amd import parameters
    assert parameters.landmarks_backend(10**6, d, 5000) == want


@pytest.mark.parametrize("d", [1, 50, 64, 65, 100, 256, 257])
def test_landmarks_backend_below_threshold_stays_on_the_host(d):
    from mellon_amd import parameters
    assert parameters.KMEANS_DEVICE_THRESHOLD == 2e8
    assert parameters.landmarks_backend(10**4, d, 5000) == "sklearn"          # 5e7 pairs
    assert parameters.landmarks_backend(40000, d, 5000) == "sklearn"          # exactly the threshold: not above it
    assert parameters.landmarks_backend(40001, d, 5000) == ("hip" if d <= 256 else "sklearn")


def test_wide_diagnostics_in_header_and_binding():
    from mellon_amd import _lib
    header = open(os.path.join(ROOT, "include", "mellon_hip.h")).read()
    declared = set(re.findall(r"^(?:int|void|const char\*)\s+(mln_\w+)\s*\(", header, flags=re.M))
    bound = {s[0]: s for s in _lib.SYMBOLS}
    for name, n_args in (("mln_diag_rowmin_wide", 13), ("mln_diag_nn_last", 2)):
        assert name in declared and name in bound
        assert len(bound[name][2]) == n_args
    assert callable(_lib.Context.diag_rowmin_wide) and callable(_lib.Context.nn_last)
