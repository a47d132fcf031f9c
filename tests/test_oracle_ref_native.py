"""`points_in_boxes_cpu` pinned by the reference's OWN compiled C++ (roiaware_pool3d.cpp:121-168):
  * tests/golden/points_in_boxes_cpu_ref.npz -- outputs of oracle/_ref (tests/golden/make_golden_ref_native.py) on random rotated boxes,
    points on the faces / inside and outside the 1e-2 margin, degenerate boxes and empty inputs;
  * tests/golden/points_in_boxes_cpu_ref_trials.npz -- outputs of oracle/_ref on five seeded random scenes, against which the C
    restatement is compared bit for bit; where oracle/_ref is built (`make -C oracle ref`), the live reference function as well."""
import os

import numpy as np
import pytest

from oracle import native as O
from oracle import ref_native as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "points_in_boxes_cpu_ref.npz")
TRIALS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "points_in_boxes_cpu_ref_trials.npz")


def _cases():
    z = np.load(GOLD)
    for k in "abcde":
        yield k, z[f"{k}_pts"], z[f"{k}_boxes"], z[f"{k}_flags"]


def test_restatement_matches_reference_vectors():
    n_set = 0
    for k, pts, boxes, flags in _cases():
        got = O.points_in_boxes_cpu(pts, boxes)
        assert got.shape == flags.shape and np.array_equal(got, flags), f"case {k}"
        n_set += int(flags.sum())
    assert n_set > 1000      # the vectors are not all-zero


def test_product_host_op_matches_reference_vectors():
    from snvc_amd import _lib
    from snvc_amd.extension.roiaware_pool3d import roiaware_pool3d_utils as U
    try:
        _lib.lib()
    except Exception as e:  # pragma: no cover - the build check runs first
        pytest.fail(f"libsnvc_hip.so did not load: {e}")
    for k, pts, boxes, flags in _cases():
        if pts.shape[0] == 0 or boxes.shape[0] == 0:
            continue
        assert np.array_equal(np.asarray(U.points_in_boxes_cpu(pts, boxes)), flags), f"case {k}"


def test_restatement_matches_live_reference():
    z = np.load(TRIALS)
    for trial in range(5):
        pts, boxes, exp = z[f"{trial}_pts"], z[f"{trial}_boxes"], z[f"{trial}_flags"]
        if R.available():
            assert np.array_equal(R.points_in_boxes_cpu(pts, boxes), exp), f"stored trial {trial}"
        assert np.array_equal(O.points_in_boxes_cpu(pts, boxes), exp), f"trial {trial}"
        assert exp.sum() > 0


@pytest.mark.skipif(not R.available(), reason="oracle/_ref not built")
def test_fixture_is_what_the_reference_build_returns():
    for k, pts, boxes, flags in _cases():
        assert np.array_equal(R.points_in_boxes_cpu(pts, boxes), flags), f"case {k}"
