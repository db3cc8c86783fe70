"""The worlds of tests/resident_state_cases.py mean what tests/test_gpu_resident_state.py takes them to mean:
a cell of that matrix only says something if state derived from the map BEFORE the change would give another
answer than the map after it. Shown here with the numpy references alone, for every mutation and both queries:
the box-max level inside the search window, the K best poses, the covariance, the prior's winner, the pose-set
scores and the ray-check records all differ between the two maps. Also: the windows of the new consumers stay
clear of the edge band on the final map (the peaks and volume references speak about no others), the prior
moves the winner off the plain arg-max, and the global_parts world reaches the three rank paths. No GPU."""
import numpy as np
import pytest

import global_map_cases as GM
import resident_state_cases as RS

NEW = ("peaks", "volume_cov", "prior", "pose_sets", "ray_check")


@pytest.fixture(scope="module", params=RS.MUTATIONS)
def kind(request, oracle):
    RS.world(request.param, oracle)
    return request.param


def test_the_matrix_is_seven_old_and_five_new_mutations():
    assert len(RS.OLD_MUTATIONS) == 7 and len(RS.NEW_MUTATIONS) == 5 and len(set(RS.MUTATIONS)) == 12
    assert set(RS.LEVEL_MUTATIONS) <= set(RS.MUTATIONS)


def test_the_cells_change(kind):
    w = RS.world(kind)
    assert w["before"].shape != w["grid"].shape or not np.array_equal(w["before"], w["grid"])
    assert len(w["queries"]) == len(w["warm"]) == len(w["queries_new"]) == len(w["warm_new"]) == 2
    assert (w["gone"] is None) == (w["qid"] == RS.MID)


@pytest.mark.parametrize("which", ["queries", "queries_new"])
def test_box_max_level_differs_inside_the_search_window(kind, which):
    """What level_for_window hands the exact pass: a level left over from the first map would not be the
    box-max of the final cells where the window reads it."""
    w = RS.world(kind)
    for q in w[which]:
        stale_q = dict(q, geom=w["warm"][0]["geom"])
        assert not np.array_equal(RS.boxmax_in_window(w["before"], stale_q), RS.boxmax_in_window(w["grid"], q))


def test_windows_stay_clear_of_the_edge_band_on_the_final_map(kind):
    for r in RS.reference(kind, "peaks") + RS.reference(kind, "prior"):
        assert r["band"] == 0


def test_peaks_differ(kind):
    for a, b in zip(RS.reference(kind, "peaks", "before"), RS.reference(kind, "peaks")):
        assert len(b["records"]) == RS.K_MAX
        assert a["records"] != b["records"]
        assert a["records"][:1] != b["records"][:1]             # the winner alone differs too


def test_covariance_differs(kind):
    for a, b in zip(RS.reference(kind, "volume_cov", "before"), RS.reference(kind, "volume_cov")):
        assert b["summary"]["moments"]["best"]["found"] == 1 and b["summary"]["moments"]["support"] > 1
        assert a["summary"]["covariance"] != b["summary"]["covariance"]
        assert a["summary"]["moments"] != b["summary"]["moments"]


def test_the_prior_moves_the_winner_and_differs(kind):
    assert np.array_equal(RS.LAMBDA, RS.LAMBDA.T) and np.linalg.eigvalsh(RS.LAMBDA).min() > 0
    for a, b in zip(RS.reference(kind, "prior", "before"), RS.reference(kind, "prior")):
        p = b["prior"]
        assert p["best"]["found"] == 1 and p["unweighted"]["found"] == 1
        assert p["best"] != p["unweighted"] and p["penalised_key"] < p["unweighted"]["key"]
        assert (p["best"]["best_x"], p["best"]["best_y"], p["best"]["best_theta"]) != \
            (p["unweighted"]["best_x"], p["unweighted"]["best_y"], p["unweighted"]["best_theta"])
        assert a["prior"] != p and a["prior"]["best"] != p["best"]


def test_pose_set_scores_and_ray_check_records_differ(kind):
    for a, b in zip(RS.reference(kind, "pose_sets", "before"), RS.reference(kind, "pose_sets")):
        assert len(b["S"]) == RS.N_POSES and max(b["K"]) > 0
        assert a["S"] != b["S"]
    for a, b in zip(RS.reference(kind, "ray_check", "before"), RS.reference(kind, "ray_check")):
        assert b["record"]["walked"] > 0 and b["record"]["usable"] < b["record"]["beams"]
        assert a["record"] != b["record"] and a["words"] != b["words"]


def test_global_parts_reaches_the_three_rank_paths(oracle):
    """Cast node by node (scratch_limit_bytes = 1) under (2, 4): the parts between them rank cells by
    counting, by sorting and by tiles. numpy's projection is good to a few hits at cell edges, so at
    least three cells each, as tests/test_cpu_global_map_cases.py asks."""
    w = RS.world("global_parts", oracle)
    assert RS.GLOBAL_RANK == (2, 4)
    total = dict.fromkeys(GM.ALL, 0)
    for nd in w["job"]["nodes"]:
        taken = GM.paths_taken(GM.hits_per_cell(dict(w["job"], nodes=[nd]), w["shape"]), RS.GLOBAL_RANK)
        assert taken["direct"] >= 3 and taken["sorted"] >= 3, taken
        for path in GM.ALL:
            total[path] += taken[path]
    assert all(total[path] >= 3 for path in GM.ALL), total


def test_field_rebuild_changes_source_and_sigma(oracle):
    w = RS.world("field_rebuild", oracle)
    assert RS.FIELD_SIGMAS[0] != RS.FIELD_SIGMAS[1] and w["before"].shape == w["grid"].shape
    assert w.get("derived_alloc_only") and np.array_equal(w["cost_alloc"], RS._derived_alloc(w["grid"]))


def test_same_hit_indices_on_the_final_map_give_other_winners():
    """What tests/test_gpu_resident_state.py asks of prepared windows: the records of the old hit indices on
    the final cells are not the old records."""
    for kind in RS.LEVEL_MUTATIONS:
        w = RS.world(kind)
        old = [r["records"][0] for r in RS.reference(kind, "peaks", "before")]
        fresh = [r["records"][0] for r in RS.reference_of("peaks", w["grid"], w["warm_new"])]
        assert all(a != b for a, b in zip(old, fresh))
        assert all(r["band"] == 0 for r in RS.reference(kind, "peaks", "before"))
