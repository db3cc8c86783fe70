"""The case table of the global map builder (tests/global_map_cases.py) really holds
what it is there for, shown with the literal CPU builder and a numpy count of the hits
per cell; the part planner csm_host_global_map_parts; and csm_host_global_scan_poses.
No GPU."""
import numpy as np
import pytest

import global_map_cases as GM
from csm_hip import api

CASES = dict(GM.build())


@pytest.fixture(scope="module")
def built(oracle):
    out = {}
    for name, case in CASES.items():
        shape, grid, stats = oracle.construct_map(case["shape"], case["map_pose"], case["nodes"])
        out[name] = (shape, grid, stats, GM.hits_per_cell(case, shape))
    return out


@pytest.mark.parametrize("name", list(GM.CASES))
def test_case_has_its_property(built, name):
    want = GM.CASES[name][1]
    shape, grid, stats, counts = built[name]
    assert grid.shape == (shape["rows"], shape["cols"]) and stats["end_missing"] == 0
    assert counts.sum() == stats["rays"]                  # every usable beam ends in one cell
    if "shape" in want:
        assert grid.shape == want["shape"]
    if "rays" in want:
        assert stats["rays"] == want["rays"]
    if want.get("has_65535"):
        assert (grid == 65535).any() and stats["oob_reads"] > 0
    if want.get("all_zero"):
        assert not grid.any()
    if "beams" in want:
        assert sum(GM.beams(CASES[name])) == want["beams"]
    if "uncertain_min" in want:
        assert GM.MB.edge_beams(CASES[name]) >= want["uncertain_min"]
    # numpy's projection is good to a few hits at cell edges: 5 % and 8 hits of margin
    if "max_hits_min" in want:
        assert counts.max() >= 1.05 * want["max_hits_min"] + 8
    if "above" in want:
        n, cells = want["above"]
        assert (counts > 1.05 * n + 8).sum() >= cells
    for rank, paths in want["paths"].items():
        taken = GM.paths_taken(counts, rank)
        for path in paths:
            assert taken[path] >= 3, (name, rank, path, taken)
        if not paths:
            assert sum(taken.values()) == 0


@pytest.mark.parametrize("name", GM.CUT)
def test_single_nodes_have_short_and_long_cells(built, name):
    """Cast node by node under (2, 4), every part ranks some cells by counting and, in the cases of
    NODE_LONG, sorts others."""
    case, shape = CASES[name], built[name][0]
    for nd in case["nodes"]:
        taken = GM.paths_taken(GM.hits_per_cell(dict(case, nodes=[nd]), shape), (2, 4))
        assert taken["direct"] >= 3, (name, taken)
        if name in GM.NODE_LONG:
            assert taken["sorted"] + taken["tiled"] >= 3, (name, taken)


def test_rank_settings_reach_every_path_and_every_split():
    """Between them the settings put a tile below, at and above a small case's lists, and the default
    split (32) between the short and the long cells of the revisited room."""
    assert GM.RANKS[0] == (0, 0) and GM.DEFAULTS == (32, 4096)
    for direct_max, tile in GM.RANKS[1:]:
        assert direct_max >= 1 and tile >= 4 and tile & (tile - 1) == 0
    assert any(set(p["paths"].get(rk, ())) == set(GM.ALL) for _, p in GM.CASES.values() for rk in GM.RANKS[1:])


def _scratch(beams, cells):
    # csm_hip.h, csm_host_map_batch_plan: one job
    return max(beams, 1) * 40 + 4 * ((11 * beams + 23) & ~3) + 12 * cells + 8 * 135


def test_parts_are_consecutive_and_within_the_limit():
    rng = np.random.RandomState(11)
    beams = [int(b) for b in rng.randint(0, 3000, 60)]
    cells = 300 * 320
    for limit in (_scratch(max(beams), cells), _scratch(4000, cells), _scratch(20000, cells) + 17,
                  _scratch(sum(beams) // 3, cells)):
        part_of, part_bytes = api.host_global_map_parts(beams, cells, limit)
        assert part_of[0] == 0 and all(b - a in (0, 1) for a, b in zip(part_of, part_of[1:]))
        assert len(part_bytes) == part_of[-1] + 1
        for p, total in enumerate(part_bytes):
            members = [k for k in range(60) if part_of[k] == p]
            held = sum(beams[k] for k in members)
            # the per-cell bytes of the whole map once per part, the rest for the part's beams
            assert total == _scratch(held, cells)
            assert total <= limit or len(members) == 1
            # closed before the node that would have taken it past the limit
            if members[-1] + 1 < 60:
                assert _scratch(held + beams[members[-1] + 1], cells) > limit
    assert len(api.host_global_map_parts(beams, cells, _scratch(sum(beams) // 3, cells))[1]) >= 3


def test_parts_limits():
    beams, cells = [1080, 1080, 90, 0, 720], 288 * 288
    part_of, part_bytes = api.host_global_map_parts(beams, cells, 1 << 40)
    assert part_of == [0] * 5 and part_bytes == [_scratch(sum(beams), cells)]
    # one node per part; the formula is the batch planner's for a one-node job
    part_of, part_bytes = api.host_global_map_parts(beams, cells, 1)
    assert part_of == [0, 1, 2, 3, 4]
    for b, total in zip(beams, part_bytes):
        assert [total] == api.host_map_batch_plan([b], [cells], 0)[1] == [_scratch(b, cells)]
    # a node that alone exceeds the limit gets a part of its own; its neighbours still share
    part_of, _ = api.host_global_map_parts([90, 5000, 90, 0, 90], cells, _scratch(300, cells))
    assert part_of == [0, 1, 2, 2, 2]
    # zero means 1 GiB
    many = [1 << 20] * 40                         # 84 bytes per beam: 12 such nodes fit, 13 do not
    assert api.host_global_map_parts(many, 0, 0) == api.host_global_map_parts(many, 0, 1 << 30)
    assert api.host_global_map_parts(many, 0, 0)[0][:14] == [0] * 12 + [1, 1]


def test_parts_cut_at_2_24_beams():
    """Synthetic beam counts only: a part never holds more than 2^24 beams, whatever the limit."""
    full = 1 << 24
    part_of, part_bytes = api.host_global_map_parts([full // 2, full // 2, 1, full, full - 1, 1, 1], 1000, 1 << 50)
    assert part_of == [0, 0, 1, 2, 3, 3, 4]
    assert part_bytes[0] == _scratch(full, 1000) and part_bytes[3] == _scratch(full, 1000)
    beams = [10_000 * 1080 // 8] * 8              # 10 000 scans of 1080 beams in eight nodes: 1.08e7 beams
    part_of, _ = api.host_global_map_parts(beams, 1 << 20, 1 << 50)
    assert part_of == [0] * 8
    part_of, _ = api.host_global_map_parts(beams * 2, 1 << 20, 1 << 50)
    assert part_of == [0] * 12 + [1] * 4


def test_parts_refusals():
    for args in (([1080], 100, -1), ([], 100, 0), ([-1], 100, 0), ([(1 << 24) + 1], 100, 0), ([1080], -1, 0),
                 ([1080], (1 << 28) + 1, 0)):
        with pytest.raises(api.CsmError) as err:
            api.host_global_map_parts(*args)
        assert err.value.code == api.L.CSM_EINVAL
    assert api.host_global_map_parts([1 << 24], 1 << 28, 0)[0] == [0]


def test_global_scan_poses_are_the_oracle_s_compound(oracle):
    rng = np.random.RandomState(5)
    for _ in range(20):
        local_map = rng.uniform(-30, 30, 3)
        local = rng.uniform(-8, 8, (17, 3))
        got = api.host_global_scan_poses(local_map, local)
        assert got.shape == (17, 3)
        for i in range(17):
            want = np.asarray(oracle.compound(local_map, local[i]), float)
            assert got[i].tobytes() == want.tobytes()
    assert api.host_global_scan_poses((1.0, 2.0, 3.0), np.zeros((0, 3))).shape == (0, 3)
