"""The case table of the many-map builder (tests/map_batch_cases.py) really holds
what it is there for, shown with the literal CPU builder; and the chunk planner
csm_host_map_batch_plan. No GPU."""
import numpy as np
import pytest

import map_batch_cases as MB
from csm_hip import api

CASES = dict(MB.build())


@pytest.mark.parametrize("name", list(MB.CASES))
def test_case_has_its_property(oracle, name):
    case, want = CASES[name], MB.CASES[name][1]
    shape, grid, stats = oracle.construct_map(case["shape"], case["map_pose"], case["nodes"])
    assert grid.shape == (shape["rows"], shape["cols"])
    assert stats["end_missing"] == 0
    if "shape" in want:
        assert grid.shape == want["shape"]
    if "rays" in want:
        assert stats["rays"] == want["rays"]
    if "updates" in want:
        assert stats["updates"] == want["updates"]
    if "updates_min" in want:
        assert want["updates_min"] <= stats["updates"] < want["updates_min"] + 200000
    if "saturated" in want:
        assert stats["oob_reads"] == want["saturated"]
    if want.get("has_65535"):
        assert (grid == 65535).any()
    if want.get("all_zero"):
        assert not grid.any()
    if "beams" in want:
        beams = sum(len(nd["ranges"]) for nd in case["nodes"])
        assert beams == want["beams"] and (name not in ("odd",) or (beams % 256 and beams % 32))
    # beams on cell edges: at least two where the table says so (more than a cap of one), none elsewhere
    if "uncertain_min" in want:
        assert MB.edge_beams(case) >= want["uncertain_min"]
    else:
        assert MB.edge_beams(case) == 0


def test_table_spans_the_sizes_the_schedule_must_balance(oracle):
    cells, rays = {}, {}
    for name, case in CASES.items():
        shape, _, stats = oracle.construct_map(case["shape"], case["map_pose"], case["nodes"])
        cells[name], rays[name] = shape["rows"] * shape["cols"], stats["rays"]
    assert max(cells.values()) > 30 * min(cells.values())
    assert min(rays.values()) == 0 and sorted(rays.values())[2] == 1 and max(rays.values()) > 20000


@pytest.mark.parametrize("name", MB.UPDATED)
def test_update_nodes_fit_then_grow(oracle, name):
    """The reference accepts both updates; the first leaves the frame as it is, the second grows it
    (tiny by 16 rows at its far side, odd by 32 rows and columns and blocks_of_4 by 12 columns at the near one)."""
    case = CASES[name]
    shape, grid, _ = oracle.construct_map(case["shape"], case["map_pose"], case["nodes"])
    own, moved = MB.update_nodes(case)
    shape1, grid1, stats1 = oracle.update_map(shape, grid, case["map_pose"], own)
    assert shape1 == shape and (stats1["row_min"], stats1["col_min"]) == (0, 0)
    assert stats1["rays"] > 0 and stats1["end_missing"] == 0
    shape2, grid2, stats2 = oracle.update_map(shape1, grid1, case["map_pose"], moved)
    assert shape2["rows"] * shape2["cols"] > shape["rows"] * shape["cols"]
    assert grid2.shape == (shape2["rows"], shape2["cols"])
    assert stats2["rays"] > 0 and stats2["end_missing"] == 0
    # towards negative indices, which shifts the carried block allocation, in two of the three
    assert ((stats2["row_min"], stats2["col_min"]) != (0, 0)) == (name != "tiny")


def test_shared_pair_holds_the_same_arrays():
    a, b = CASES["shared_a"], CASES["shared_b"]
    assert a["map_pose"] != b["map_pose"]
    for na, nb in zip(a["nodes"], b["nodes"]):
        assert na["angles"] is nb["angles"] and na["ranges"] is nb["ranges"]


def _scratch(beams, cells):
    # csm_hip.h, csm_host_map_batch_plan
    return max(beams, 1) * 40 + 4 * ((11 * beams + 23) & ~3) + 12 * cells + 8 * 135


def test_plan_cuts_consecutive_chunks_within_the_limit():
    rng = np.random.RandomState(7)
    beams = [int(b) for b in rng.randint(0, 30000, 40)]
    cells = [int(c) for c in rng.randint(1, 400000, 40)]
    need = [_scratch(b, c) for b, c in zip(beams, cells)]
    for limit in (max(need), 2 * max(need), 5 * max(need) + 17, sum(need) // 3):
        chunk_of, chunk_bytes = api.host_map_batch_plan(beams, cells, limit)
        assert chunk_of[0] == 0 and all(b - a in (0, 1) for a, b in zip(chunk_of, chunk_of[1:]))
        assert len(chunk_bytes) == chunk_of[-1] + 1
        for c, total in enumerate(chunk_bytes):
            members = [j for j in range(40) if chunk_of[j] == c]
            assert total == sum(need[j] for j in members)
            assert total <= limit or len(members) == 1
            # greedy: the next job would not have fitted
            if members[-1] + 1 < 40:
                assert total + need[members[-1] + 1] > limit
    assert len(api.host_map_batch_plan(beams, cells, sum(need) // 3)[1]) >= 3


def test_plan_limits():
    beams, cells = [1080 * 10, 90, 0, 720 * 30], [288 * 288, 48 * 48, 48 * 48, 160 * 176]
    need = [_scratch(b, c) for b, c in zip(beams, cells)]
    chunk_of, chunk_bytes = api.host_map_batch_plan(beams, cells, 1 << 40)
    assert chunk_of == [0, 0, 0, 0] and chunk_bytes == [sum(need)]
    chunk_of, chunk_bytes = api.host_map_batch_plan(beams, cells, min(need) - 1)
    assert chunk_of == [0, 1, 2, 3] and chunk_bytes == need
    # a job that alone exceeds the limit gets a chunk of its own; its neighbours still share
    chunk_of, _ = api.host_map_batch_plan(beams, cells, need[1] + need[2])
    assert chunk_of == [0, 1, 1, 2]
    # zero means 1 GiB
    big_cells = [(1 << 30) // 12 // 2] * 3          # two such jobs do not fit into 1 GiB, one does
    assert api.host_map_batch_plan([0] * 3, big_cells, 0) == api.host_map_batch_plan([0] * 3, big_cells, 1 << 30)
    assert api.host_map_batch_plan([0] * 3, big_cells, 0)[0] == [0, 1, 2]
    assert api.host_map_batch_plan([0] * 3, [c // 2 - 1000 for c in big_cells], 0)[0] == [0, 0, 0]
    with pytest.raises(api.CsmError):
        api.host_map_batch_plan(beams, cells, -1)
    with pytest.raises(api.CsmError):
        api.host_map_batch_plan([], [], 0)
    with pytest.raises(api.CsmError):
        api.host_map_batch_plan([-1], [10], 0)
