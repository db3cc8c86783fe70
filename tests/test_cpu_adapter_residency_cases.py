"""The inputs of tests/adapter_residency_cases.py mean what tests/test_gpu_adapter_residency.py takes them to
mean: that test tells the cells a C++ adapter holds on the device by the row it returns, which only works if
grid A and grid B give different rows for the same scan. Shown here on the CPU for every matcher of the test:
the grid search through the oracle's literal loops, the hill climbing through the library's host restatement,
the correlative paths (and the branch-and-bound detector) through the oracle. No GPU."""
import numpy as np

import adapter_residency_cases as AR
from csm_hip import api


def test_the_grids_share_shape_and_geometry_and_are_small():
    c = AR.case()
    assert c["A"].shape == c["B"].shape == (AR.ROWS, AR.COLS) == (200, 200)
    assert (c["A"] != c["B"]).any() and c["A"].size % 4 == 0         # the driver's doubles stay aligned
    assert len(c["angles"]) == len(c["ranges"]) == AR.N_BEAMS


def test_grid_search_differs_on_a_small_window(oracle):
    a, b = (oracle.grid_search(AR.on(AR.case()[k]), *AR.GRID_SEARCH) for k in "AB")
    # the offsets are accumulated doubles: a loop may end one step short of its 11
    assert 10 ** 3 <= a["evaluations"] == b["evaluations"] <= 11 ** 3
    assert a["found"] == 1 and b["found"] == 1
    assert a["estimatedPose"] != b["estimatedPose"] and a["scoreMax"] != b["scoreMax"]


def test_hill_climbing_differs():
    c = AR.case()
    a, b = (api.host_hill_climbing(c[k], c["geom"], c["angles"], c["ranges"], c["rel_pose"], c["init_pose"],
                                   *AR.HILL, greedy=AR.GREEDY) for k in "AB")
    assert a["estimated_pose"] != b["estimated_pose"] and a["normalized_cost"] != b["normalized_cost"]
    assert not np.array_equal(a["covariance"], b["covariance"])


def test_correlative_matcher_differs(oracle):
    a, b = (oracle.csm(AR.on(AR.case()[k]), *AR.CSM) for k in "AB")
    assert a["found"] == 1 and b["found"] == 1
    assert a["estimatedPose"] != b["estimatedPose"] and a["scoreMax"] != b["scoreMax"]


def test_detectors_find_a_pose_on_a_that_b_does_not_give(oracle):
    init = AR.detector_init_pose()
    assert np.allclose(init, AR.case()["init_pose"], atol=1e-12)
    for fn, prm in ((oracle.csm, AR.LDC), (oracle.bnb, AR.BNB)):
        a, b = (fn(dict(AR.on(AR.case()[k]), init_pose=init), *prm) for k in "AB")
        assert a["found"] == 1
        assert (b["found"], b["estimatedPose"], b["scoreMax"]) != (1, a["estimatedPose"], a["scoreMax"])
