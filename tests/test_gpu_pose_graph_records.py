"""The device results of the pose-graph unit, pinned: the built library must reproduce, bit for bit, what
tests/golden/pose_graph_records.json records for the seeded cases of tests/pose_graph_record_cases.py (poses,
errors, lambdas, every trace field, every entry of every marginal block, as float.hex() strings). The parity
tests (test_gpu_pose_graph*.py) hold the device to the host within tolerances; a change of the reduction shape,
of a summation order or of a launch chain can stay inside them. Here it changes a string."""
import json
import os

import pytest

import pose_graph_record_cases as cases

pytestmark = pytest.mark.gpu

LM_IDS = ["%s-%s" % c for c in cases.LM_CASES]
STOP_IDS = ["%s-row%d" % (s, cases.STOP_ROW) for s in cases.SOLVERS]


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(os.path.dirname(__file__), "golden", "pose_graph_records.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def recomputed(gpu_ctx):
    return cases.record(gpu_ctx)


@pytest.mark.parametrize("case", LM_IDS)
def test_lm_result_equals_the_record(recorded, recomputed, case):
    assert recomputed["lm"][case] == recorded["lm"][case]


@pytest.mark.parametrize("case", STOP_IDS)
def test_launches_after_the_stop_change_nothing(recorded, recomputed, case):
    """iterations_max = the steps the case takes against iterations_max = 10: the same result"""
    assert recomputed["lm_at_its_steps"][case] == recorded["lm_at_its_steps"][case]
    assert recomputed["lm_at_its_steps"][case] == recomputed["lm"][case]


@pytest.mark.parametrize("name", cases.BLOCKED)
def test_marginals_equal_the_record(recorded, recomputed, name):
    assert recomputed["marginals"][name] == recorded["marginals"][name]


def test_the_record_is_not_vacuous(recorded):
    assert sorted(recorded["lm"]) == sorted(LM_IDS) and sorted(recorded["lm_at_its_steps"]) == sorted(STOP_IDS)
    for name in cases.BLOCKED:
        c = cases.graph(name)[0]
        assert 3 * len(c["local"]) > 96                  # the blocked factorization, not the single workgroup
        assert len(recorded["lm"]["schur-" + name]["local"]) == 3 * len(c["local"])
        assert cases.last_scan_with_edges(c) == len(c["scan"]) - 1
        assert all(p["finite"] == 1 for p in recorded["marginals"][name]["pairs"])
    assert 3 * (len(cases.graph("wide765")[0]["local"]) + len(cases.graph("wide765")[0]["scan"])) == 765
    for solver in cases.SOLVERS:
        stop = recorded["lm"]["%s-row%d" % (solver, cases.STOP_ROW)]
        assert 1 < stop["steps"] < 10 and len(stop["trace"]) == stop["steps"]
        assert recorded["lm_at_its_steps"]["%s-row%d" % (solver, cases.STOP_ROW)]["steps"] == stop["steps"]
        zero = recorded["lm"]["%s-row%d" % (solver, cases.ZERO_ROW)]
        assert zero["trace"] and all(float.fromhex(t["rhs_norm2"]) == 0.0 for t in zero["trace"])
    assert recorded["lm"]["cg-wide765"]["cg_iterations"] > 0
    assert all(recorded["lm"]["schur-" + n]["cg_iterations"] == 0 for n in cases.BLOCKED)
    pairs33 = cases.marginal_pairs("local33")
    assert pairs33[0] == (0, None) and pairs33[1] == (32, len(cases.graph("local33")[0]["scan"]) - 1)
    assert recorded["marginals"]["dense49"]["n_columns"] == 49 == len(recorded["marginals"]["dense49"]["pairs"])
    assert len(recorded["marginals"]["local33"]["pairs"]) == 3
