"""The crafted cases of tests/map_rank_cases.py hold their properties, shown with the literal CPU builder
and oracle.bayes_update: every cell of the oracle's map is the value of its own sequence of hits and misses,
every target has exactly its planned sequence, and a target's value changes whenever its miss block lands
in another interval between its hits. Also the exact numbers of hit cells per rank path that
tests/test_gpu_map_rank.py asserts. No GPU."""
import numpy as np
import pytest

import global_map_cases as GM
import map_rank_cases as MR

CASES = dict(MR.build())
RANKED = {name: [c["rank"]] if "rank" in c else GM.RANKS for name, c in CASES.items() if c["targets"]}


@pytest.fixture(scope="module")
def built(oracle):
    """name -> (shape, grid, stats, sequences), computed once and never changed."""
    out = {}
    for name, case in CASES.items():
        shape, grid, stats = oracle.construct_map(case["shape"], case["map_pose"], case["nodes"], **MR.oracle_kw(case))
        grid.setflags(write=False)
        out[name] = (shape, grid, stats, MR.cell_sequences(case, shape))
    return out


def test_the_table_holds_every_family():
    names = list(CASES)
    assert names[:MR.SWEEP_BUILDS] == ["sweep_%d" % b for b in range(MR.SWEEP_BUILDS)]
    assert names[MR.SWEEP_BUILDS:] == ["boundaries_default", "largest_tile", "all_pairs", "two_nodes", "walks_1",
                                       "walks_100"]
    for case in CASES.values():
        assert case["shape"]["res"] == 0.25 and (case["prob_hit"], case["prob_miss"]) == (0.52, 0.1)
        assert all(len(nd["angles"]) == len(nd["ranges"]) > 0 for nd in case["nodes"])


def test_the_block_reaches_the_floor_and_the_hits_keep_climbing():
    """The two facts the construction rests on, measured: so many misses take EVERY value to the fixed
    point 1, and from 1 so many hits give values that are new each time and below 65535 (at 65535 the tails run together)."""
    hit, miss = MR.update_tables(MR.PROB_HIT, MR.PROB_MISS)
    assert miss[1] == 1
    v, floor_after = np.arange(65536), 0
    while (v != 1).any():
        v = miss[v]
        floor_after += 1
        assert floor_after <= 64
    seen, v, steps = {1}, int(hit[1]), 0
    while v != 65535 and v not in seen:
        seen.add(v)
        steps += 1
        v = int(hit[v])
    assert v == 65535                    # ... where every longer tail ends as well: it names nothing
    print("misses to the floor from any value: %d; hits from 1 that each give a new value below 65535: %d "
          "(%d distinct values, the floor included)" % (floor_after, steps, len(seen)))
    assert floor_after <= MR.BLOCK
    tails = [n - k for case in CASES.values() for _, n, k in case["targets"] if k is not None]
    assert steps >= MR.MAX_TAIL >= max(tails)
    # the tables are the oracle's single updates
    assert MR.value_of("H") == hit[0] and MR.value_of("M") == miss[0] and MR.value_of("HMH") == hit[miss[hit[0]]]


@pytest.mark.parametrize("name", list(CASES))
def test_every_cell_is_the_value_of_its_own_sequence(built, name):
    shape, grid, stats, seqs = built[name]
    assert stats["end_missing"] == 0
    assert stats["updates"] == sum(len(s) for s in seqs.values())
    assert stats["rays"] == sum(s.count("H") for s in seqs.values())
    want = np.zeros_like(grid)
    values = {}
    for (x, y), s in seqs.items():
        assert 0 <= x < shape["cols"] and 0 <= y < shape["rows"]
        if s not in values:
            values[s] = MR.value_of(s) if len(s) <= 400 else None
        if values[s] is None:            # the long lists: through the tables
            hit, miss = MR.update_tables(MR.PROB_HIT, MR.PROB_MISS)
            v = 0
            for letter in s:
                v = int(hit[v] if letter == "H" else miss[v])
            values[s] = v
        want[y, x] = values[s]
    bad = np.argwhere(want != grid)
    assert bad.size == 0, (name, len(bad), bad[:5])
    assert max(shape["rows"], shape["cols"]) <= 400


@pytest.mark.parametrize("name", list(CASES))
def test_every_beam_is_usable_and_far_from_an_edge(built, name):
    """No beam ends within a thousandth of a sub-pixel of a sub-pixel edge (the ends are centres), so the
    device certifies every projection."""
    case, shape = CASES[name], built[name][0]
    assert len(MR.rays_of(case, shape)) == sum(len(nd["ranges"]) for nd in case["nodes"])
    scaled = shape["res"] / case["subpixel_scale"]
    for nd in case["nodes"]:
        x, y, th = nd["pose"]
        for p, off in ((x + nd["ranges"] * np.cos(th + nd["angles"]), shape["off_x"]),
                       (y + nd["ranges"] * np.sin(th + nd["angles"]), shape["off_y"])):
            frac = (p - off) / scaled % 1.0
            assert np.abs(frac - 0.5).max() < 1e-3


@pytest.mark.parametrize("name", list(RANKED))
def test_targets_have_exactly_their_planned_sequence(built, name):
    case = CASES[name]
    shape, grid, _, seqs = built[name]
    cells = [MR.in_frame(T, shape) for T, _, _ in case["targets"]]
    assert len(set(cells)) == len(cells)
    for cell, (T, n, k) in zip(cells, case["targets"]):
        assert seqs[cell] == MR.planned(n, k), (name, T, n, k, seqs[cell][:80])
        assert seqs[cell].count("H") == n


@pytest.mark.parametrize("name", list(RANKED))
def test_another_block_position_gives_another_value(built, name):
    case = CASES[name]
    shape, grid, _, _ = built[name]
    by_n = {}
    for T, n, k in case["targets"]:
        if k is None:
            continue
        assert 0 <= k <= n and n - k <= MR.MAX_TAIL
        if n not in by_n:
            by_n[n] = MR.values_by_block_position(n)
        values = by_n[n]
        x, y = MR.in_frame(T, shape)
        assert grid[y, x] == values[k], (name, T, n, k)
        assert (values != values[k]).sum() == n, (name, T, n, k)
        if n <= 64:
            assert values[k] == MR.value_of(MR.planned(n, k))


def test_the_sweep_holds_every_count_and_position(built):
    specs = sorted((n, k) for name, c in CASES.items() if name.startswith("sweep") for _, n, k in c["targets"])
    assert specs == [(n, k) for n in range(1, 51) for k in range(n + 1)]
    for direct_max, tile in GM.RANKS[1:]:
        for edge in (direct_max, direct_max + 1, tile, tile + 1, 3 * tile + 1):
            assert edge <= 50 or (direct_max, tile) == (1, 64)
    # between them the builds rank by counting under every setting (a build need not: n <= 2 is rare)
    for rank in GM.RANKS:
        assert sum(MR.rank_info(c, built[name][0], rank)["direct_cells"] for name, c in CASES.items()
                   if name.startswith("sweep")) >= 2
    bounds = {n for _, n, _ in CASES["boundaries_default"]["targets"]}
    assert bounds == {32, 33, 4095, 4096, 4097} and GM.DEFAULTS == (32, 4096)
    assert {n for _, n, _ in CASES["largest_tile"]["targets"]} == {16384, 16385, 100}


def _hits(seqs):
    return np.sort(np.array([s.count("H") for s in seqs.values() if "H" in s]))


# the hit cells per rank path, case by case: what the device must report, to the cell
RANK_INFO = {
    "boundaries_default": {(32, 4096): dict(direct_cells=18, sorted_cells=9, tiled_cells=3, max_hits_per_cell=4097)},
    "largest_tile": {(32, 16384): dict(direct_cells=5, sorted_cells=3, tiled_cells=2, max_hits_per_cell=16385)},
    "all_pairs": {(1, 64): dict(direct_cells=0, sorted_cells=150, tiled_cells=0, max_hits_per_cell=2)},
}


@pytest.mark.parametrize("name", list(RANKED))
def test_rank_paths_are_counted_exactly(built, name):
    """MR.rank_info (which the GPU test asserts) is GM.paths_taken on the exact hit counts of the
    sequences, the U cells and every other cell with a hit included; every setting of the sweep reaches
    all the paths it can."""
    case = CASES[name]
    shape, _, _, seqs = built[name]
    counts = _hits(seqs)
    assert np.array_equal(counts, MR.hit_counts(case, shape))
    for rank in RANKED[name]:
        taken = GM.paths_taken(counts, rank)
        info = MR.rank_info(case, shape, rank)
        assert info == dict(direct_cells=taken["direct"], sorted_cells=taken["sorted"], tiled_cells=taken["tiled"],
                            max_hits_per_cell=counts.max())
        assert sum(taken.values()) == len(counts)
        if name in RANK_INFO:
            assert info == RANK_INFO[name][rank]
        if name.startswith("sweep"):
            tiled = {(0, 0): 0, (2, 4): 1, (8, 16): 1, (1, 64): 0}[rank]
            assert taken["sorted"] > 0 and (taken["tiled"] > 0) == bool(tiled)
    # one node per part: a cell is counted in every part that hits it
    parts = [[k] for k in range(len(case["nodes"]))]
    info = MR.rank_info(case, shape, (2, 4), parts)
    whole = MR.rank_info(case, shape, (2, 4))
    total = lambda i: i["direct_cells"] + i["sorted_cells"] + i["tiled_cells"]
    if name == "two_nodes":
        split = sum(1 for _, n, k in case["targets"] if 0 < k < n)
        assert split > 0 and total(info) == total(whole) + split
    else:
        assert info == whole


def test_all_pairs_fills_the_hit_cell_list(built):
    case = CASES["all_pairs"]
    shape, _, stats, seqs = built["all_pairs"]
    rays = sum(len(nd["ranges"]) for nd in case["nodes"])
    counts = _hits(seqs)
    assert stats["rays"] == rays and len(counts) * 2 == rays and (counts == 2).all()
    # under rank_direct_max = 1: hit cells + long cells = rays, and the launch bound usable / 2 is the count
    long_cells = int((counts > 1).sum())
    assert len(counts) + long_cells == rays and rays // 2 == long_cells


def test_two_nodes_splits_every_target_over_the_parts(built):
    case = CASES["two_nodes"]
    shape = built["two_nodes"][0]
    rays = MR.rays_of(case, shape)
    for T, n, k in case["targets"]:
        cell = MR.in_frame(T, shape)
        assert [r["node"] for r in rays if r["H"] == cell] == [0] * k + [2] * (n - k)
        assert [r["node"] for r in rays if cell in r["cells"]] == [1] * MR.BLOCK
    assert len({nd["pose"] for nd in case["nodes"]}) == 3
    # node 0 alone leaves the frame of the whole case: the updates of the GPU test need no resize
    from oracle import oracle as O
    first = O.construct_map(case["shape"], case["map_pose"], case["nodes"][:1], **MR.oracle_kw(case))
    assert first[0] == shape
    grid, frame = first[1], first[0]
    for nd in case["nodes"][1:]:
        frame, grid, _ = O.update_map(frame, grid, case["map_pose"], nd, **MR.oracle_kw(case))
        assert frame == shape
    assert np.array_equal(grid, built["two_nodes"][1])


@pytest.mark.parametrize("scale", MR.WALK_SCALES)
def test_walks_hold_every_named_walk(built, scale):
    case = CASES["walks_%d" % scale]
    shape = built[case["name"]][0]
    rays = MR.rays_of(case, shape)
    full = [r["cells"] + [r["H"]] for r in rays]           # the end cell is the hit cell here
    for r, cells in zip(rays, full):
        assert (r["e"][0] // scale, r["e"][1] // scale) == r["H"] and len(set(cells)) == len(cells)
    cols = [len({x for x, _ in c}) for c in full]
    rows = [len({y for _, y in c}) for c in full]
    up = [r["e"][1] > r["s"][1] for r in rays]
    assert any(c == 1 and len(f) > 8 and u for c, f, u in zip(cols, full, up))
    assert any(c == 1 and len(f) > 8 and not u for c, f, u in zip(cols, full, up))
    assert any(w == 1 and c > 8 and r["e"][0] > r["s"][0] for w, c, r in zip(rows, cols, rays))
    assert any(w == 1 and c > 8 and r["e"][0] < r["s"][0] for w, c, r in zip(rows, cols, rays))
    # through exact corners: every step of the walk is diagonal
    pure = [f for f in full if len(f) > 5 and all(a[0] != b[0] and a[1] != b[1] for a, b in zip(f, f[1:]))]
    assert sum(1 for f in pure if (f[-1][1] - f[0][1]) * (f[-1][0] - f[0][0]) > 0) == 2      # rising, both ways
    assert sum(1 for f in pure if (f[-1][1] - f[0][1]) * (f[-1][0] - f[0][0]) < 0) == 2      # falling
    assert any(c == 2 and len(f) > 64 for c, f in zip(cols, full))
    assert any(c > 64 and u for c, u in zip(cols, up)) and any(c > 64 and not u for c, u in zip(cols, up))
    assert sum(1 for r in rays if r["s"][0] > r["e"][0]) >= 6
