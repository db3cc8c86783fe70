"""The decisions of the projection certificate, pinned: the built library must list,
flag and hand to the host exactly what tests/golden/certificate_records.json records for the seeded cases of
tests/certificate_cases.py. The parity tests only ask that every mismatch is listed; a margin that became looser
in one kernel would pass them until an unlucky beam arrived, and one that became wider would only cost time.
Here either changes a list or a count."""
import json
import os

import pytest

import certificate_cases as cases

pytestmark = pytest.mark.gpu

FAMILIES = ("project_scan", "pose_sets", "ray_check", "greedy_cost", "hill_climbing", "map_build")


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(os.path.dirname(__file__), "golden", "certificate_records.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def recomputed(gpu_ctx):
    return cases.record(gpu_ctx)


@pytest.mark.parametrize("family", FAMILIES)
def test_decisions_equal_the_record(recorded, recomputed, family):
    assert recomputed[family] == recorded[family]


def test_the_record_is_not_vacuous(recorded):
    """The aligned frame puts hit points on cell edges: every family hands something to the host there, and
    the generic frame lists next to nothing (the bound of tests/test_gpu_projection.py)."""
    scan = recorded["project_scan"]
    assert scan["aligned"]["count"] == len(scan["aligned"]["uncertified"]) > 0
    assert recorded["pose_sets"]["aligned"]["uncertain_poses"] == len(recorded["pose_sets"]["aligned"]["flagged"]) > 0
    assert recorded["ray_check"]["aligned"]["host_beams"] > 0
    assert recorded["greedy_cost"]["aligned"]["host_path"] == 1
    assert recorded["hill_climbing"]["aligned"]["host_path"] == 1
    assert recorded["map_build"]["aligned"]["least_cap"] > 1
    assert recorded["map_build"]["aligned"]["device_projection_below"] == 0
    for name in cases.FRAMES:
        assert scan[name]["count"] == len(scan[name]["uncertified"])       # nothing overflowed
        assert scan[name]["entries"] == (2 * cases.WIN_THETA + 1) * cases.N_BEAMS
    assert len(scan["generic"]["uncertified"]) < scan["generic"]["entries"] // 1000
