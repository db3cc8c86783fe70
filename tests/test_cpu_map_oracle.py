"""CPU checks of the map-building restatement (oracle/map_oracle.cpp): the
step-by-step ray walk against an independent closed form, the binary-Bayes cell
update, and the resize geometry."""
import json
import math
import os
import struct

import numpy as np
import pytest

from csm_hip import synth

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def unhex(h):
    return struct.unpack(">d", bytes.fromhex(h))[0]


def test_bayes_primitives_bit_exact_vs_reference(oracle):
    """The conversions the cell update is made of, against outputs of the
    reference's own inline functions (grid_map_new/grid_values.hpp:11-58, built
    into oracle/_ref; tests/golden/ref_geometry.json)."""
    with open(os.path.join(GOLD, "ref_geometry.json")) as f:
        gold = json.load(f)
    lib = oracle.lib()
    for v, h in gold["value_to_odds"]:
        assert lib.orc_bb_value_to_odds(v) == unhex(h)
    for h, v in gold["probability_to_value"]:
        assert lib.orc_bb_probability_to_value(unhex(h)) == v
    for h, o in gold["probability_to_odds"]:
        assert lib.orc_bb_probability_to_odds(unhex(h)) == unhex(o)
    for h, p in gold["odds_to_probability"]:
        want = min(max(unhex(p), 1e-3), 1.0 - 1e-3)      # the wrapper's clamp, grid_binary_bayes.cpp:380
        assert lib.orc_bb_odds_to_probability(unhex(h)) == want


def test_bayes_primitives_against_live_reference_library(oracle):
    ref = oracle.ref()
    if ref is None or not hasattr(ref, "ref_value_to_odds"):
        pytest.skip("oracle/_ref not built (no /root/reference on this machine)")
    lib = oracle.lib()
    for v in range(1, 65535):
        assert lib.orc_bb_value_to_odds(v) == ref.ref_value_to_odds(v)
    for p in np.linspace(1e-3, 1.0 - 1e-3, 20001):
        assert lib.orc_bb_probability_to_value(float(p)) == ref.ref_probability_to_value(float(p))


def closed_form_cells(sx, sy, ex, ey, s):
    """Per-column closed form of the sub-pixel ray walk: with N the ray's height
    in units of 1/(2 s dx) cell, column j holds the rows between its entry and
    exit heights; a ray through an exact cell corner steps diagonally."""
    if sx > ex:
        sx, sy, ex, ey = ex, ey, sx, sy
    X0, Y0, X1, Y1 = sx // s, sy // s, ex // s, ey // s
    if X0 == X1:
        return {(X0, y) for y in range(min(Y0, Y1), max(Y0, Y1) + 1)}
    dx, dy = ex - sx, ey - sy
    den = 2 * s * dx
    n = Y0 * den + (2 * (sy % s) + 1) * dx
    first = 2 * s - (2 * (sx % s) + 1)
    last = 2 * (ex % s) + 1
    m = X1 - X0
    cells = set()
    enter = Y0
    for j in range(m + 1):
        n_out = n + dy * (first + 2 * s * j) if j < m else n + dy * (first + 2 * s * (m - 1) + last)
        if dy > 0:
            top = -(-n_out // den) - 1
            cells.update((X0 + j, r) for r in range(enter, top + 1))
            enter = n_out // den
        else:
            bot = n_out // den
            cells.update((X0 + j, r) for r in range(bot, enter + 1))
            enter = -(-n_out // den) - 1
    return cells


def test_ray_walk_matches_closed_form(oracle):
    rng = np.random.RandomState(0)
    for scale in (1, 2, 3, 4, 100):
        for _ in range(1500):
            hi = 40 * scale
            sx, sy, ex, ey = (int(v) for v in rng.randint(0, hi, 4))
            walk = oracle.ray_cells(sx, sy, ex, ey, scale)
            assert len(set(walk)) == len(walk)                       # no cell twice
            assert set(walk) == closed_form_cells(sx, sy, ex, ey, scale), (sx, sy, ex, ey, scale)
            assert (sx // scale, sy // scale) in walk and (ex // scale, ey // scale) in walk
            for a, b in zip(walk, walk[1:]):                         # 8-connected, one step at a time
                assert max(abs(a[0] - b[0]), abs(a[1] - b[1])) == 1


def test_ray_walk_corner_cases(oracle):
    # through exact cell corners (scale 1: sub-pixel centres at .5): diagonal steps
    assert oracle.ray_cells(0, 0, 3, 3, 1) == [(0, 0), (1, 1), (2, 2), (3, 3)]
    assert oracle.ray_cells(3, 3, 0, 0, 1) == [(0, 0), (1, 1), (2, 2), (3, 3)]      # swapped ends
    assert oracle.ray_cells(0, 3, 3, 0, 1) == [(0, 3), (1, 2), (2, 1), (3, 0)]
    assert oracle.ray_cells(2, 5, 2, 1, 1) == [(2, 1), (2, 2), (2, 3), (2, 4), (2, 5)]   # vertical
    assert oracle.ray_cells(1, 4, 6, 4, 1) == [(x, 4) for x in range(1, 7)]            # horizontal
    assert oracle.ray_cells(7, 7, 7, 7, 1) == [(7, 7)]
    # same full-pixel column at sub-pixel scale takes the vertical branch
    assert oracle.ray_cells(110, 120, 190, 480, 100) == [(1, y) for y in range(1, 5)]


def test_bayes_update_table(oracle):
    hit, miss = 0.62, 0.46
    v0 = oracle.bayes_update(0, hit)
    assert v0 == int(1 + (hit - 1e-3) * 65534.0 / (1.0 - 1e-3 - 1e-3))
    assert oracle.bayes_update(0, miss) < 32768 < v0
    # repeated hits climb to ValueMax = 65535 in about 13 steps and stay there.
    # NOTE: the reference's odds table has 65535 entries (grid_values.cpp:74-77),
    # so its next update of such a cell reads one entry past the end (undefined
    # behaviour); the restatement extends the table's formula to 65535 and counts
    # those reads (stats["oob_reads"]). Repeated misses fall to 1.
    v, seen = v0, 0
    for _ in range(200):
        nv = oracle.bayes_update(v, hit)
        assert nv >= v
        seen += nv != v
        v = nv
    assert v == oracle.bayes_update(v, hit) == 65535 and seen < 20
    assert oracle.bayes_update(65535, miss) < 65535
    v = oracle.bayes_update(0, miss)
    for _ in range(200):
        nv = oracle.bayes_update(v, miss)
        assert nv <= v
        v = nv
    assert v == 1
    # hit then miss differs from miss then hit somewhere: order matters
    diff = sum(oracle.bayes_update(oracle.bayes_update(u, hit), miss) !=
               oracle.bayes_update(oracle.bayes_update(u, miss), hit) for u in range(1, 65535, 97))
    assert diff > 0


def test_construct_map_geometry_and_content(oracle):
    case = synth.map_case(3, n_scans=4, n_beams=360)
    shape, grid, stats = oracle.construct_map(case["shape"], case["map_pose"], case["nodes"])
    assert stats["end_missing"] == 0
    assert stats["rays"] > 0.9 * 4 * 360 - 8
    assert shape["rows"] % 16 == 0 and shape["cols"] % 16 == 0
    # the offset moved by whole blocks of the ORIGINAL frame (offset 0)
    assert abs(shape["off_x"] / (16 * 0.05) - round(shape["off_x"] / (16 * 0.05))) < 1e-9
    assert grid.shape == (shape["rows"], shape["cols"])
    known = grid != 0
    assert 0.05 < known.mean() < 0.9
    assert (grid[known] > 40000).sum() > 100 and (grid[known] < 30000).sum() > 1000
    # every hit point lies inside the map with the one-cell margin of Resize
    ys, xs = np.nonzero(known)
    assert xs.min() >= 1 and ys.min() >= 1 and xs.max() <= shape["cols"] - 2 and ys.max() <= shape["rows"] - 2
    # IndexToBlock sends a negative index one block further than floor would
    # (grid_map.cpp:809-812), so the first resize out of the original frame
    # keeps a spare block row / column; from a frame where every index is
    # non-negative the same scans give the tight box, and that one is stable
    shape2, grid2, _ = oracle.construct_map(shape, case["map_pose"], case["nodes"])
    assert shape2["rows"] == shape["rows"] - 16 and shape2["cols"] == shape["cols"] - 16
    shape3, grid3, _ = oracle.construct_map(shape2, case["map_pose"], case["nodes"])
    assert shape3 == shape2 and np.array_equal(grid2, grid3)
    # same cells, shifted by the spare block
    dy = int(round((shape2["off_y"] - shape["off_y"]) / 0.05))
    dx = int(round((shape2["off_x"] - shape["off_x"]) / 0.05))
    assert np.array_equal(grid[dy:dy + shape2["rows"], dx:dx + shape2["cols"]], grid2)


def test_construct_map_respects_usable_range(oracle):
    case = synth.map_case(5, n_scans=2, n_beams=180)
    _, _, full = oracle.construct_map(case["shape"], case["map_pose"], case["nodes"])
    _, _, short = oracle.construct_map(case["shape"], case["map_pose"], case["nodes"], usable_max=2.0)
    assert 0 < short["rays"] < full["rays"]


def _map_cases():
    with open(os.path.join(GOLD, "map_cases.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("rec", _map_cases(), ids=lambda r: r["name"])
def test_map_golden(oracle, rec):
    """Regression pin of the restatement (tests/golden/map_cases.json)."""
    kw = dict(rec["synth"])
    if "rel_pose" in kw:
        kw["rel_pose"] = tuple(kw["rel_pose"])
    case = synth.map_case(**kw)
    shape, grid, stats = oracle.construct_map(case["shape"], case["map_pose"], case["nodes"], **rec["builder"])
    h = 1469598103934665603
    for b in grid.astype("<u2").tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    want = rec["batch"]
    assert "%016x" % h == want["hash"]
    assert (shape["rows"], shape["cols"], stats["rays"], stats["updates"], stats["oob_reads"]) == \
        (want["rows"], want["cols"], want["rays"], want["updates"], want["saturated"])
    assert [shape["off_x"], shape["off_y"]] == [unhex(v) for v in want["off"]]


# ---------------------------------------------------------------- block allocation


def test_block_move_by_hand(oracle):
    """GridMap::Resize's block move on the bitmap: shifts in both directions, and a shrink that
    drops the blocks outside the new map."""
    old = np.arange(1, 13, dtype=np.uint8).reshape(3, 4)
    shape = dict(res=0.05, off_x=0.0, off_y=0.0, rows=48, cols=64, log2_block=4)
    grown = dict(shape, rows=80, cols=96)
    # the new map starts one block row below and two block columns left of the old one
    got = oracle.move_blocks(old, shape, grown, -16, -32)
    want = np.zeros((5, 6), np.uint8)
    want[1:4, 2:6] = old
    assert np.array_equal(got, want)
    # ... and one block row above / one block column right of it: a shift the other way
    moved = dict(shape, rows=32, cols=64)
    got = oracle.move_blocks(old, shape, moved, 16, 16)
    want = np.zeros((2, 4), np.uint8)
    want[:, :3] = old[1:, 1:]
    assert np.array_equal(got, want)
    # a shrink to the middle block: everything else is dropped
    small = dict(shape, rows=16, cols=16)
    assert np.array_equal(oracle.move_blocks(old, shape, small, 16, 16), old[1:2, 1:2])
    # nothing allocated before: nothing after
    assert not oracle.move_blocks(None, shape, grown, -16, -32).any()


@pytest.mark.parametrize("log2_block", [2, 3, 4, 5])
def test_construct_map_tracks_allocation(oracle, log2_block):
    """A fresh construct allocates exactly the blocks holding a known cell; a rebuild from other
    scans moves the old blocks (shift in either direction), keeps the overlapping ones allocated
    with their cells reset, and every known cell lies in an allocated block."""
    from cost_edge_cases import initial_shape
    case = synth.map_case(5, n_scans=16, n_beams=360, step=0.2)
    nodes = case["nodes"]
    shape0 = initial_shape(0.05, log2_block)
    shape1, grid1, st1 = oracle.construct_map(shape0, nodes[0]["pose"], nodes[:6])
    assert np.array_equal(st1["alloc"], oracle.derived_alloc(grid1, log2_block))
    assert st1["alloc"].shape == (shape1["rows"] >> log2_block, shape1["cols"] >> log2_block)
    reset_but_allocated = 0
    shape, grid, alloc = shape1, grid1, st1["alloc"]
    for lo, hi in ((8, 16), (0, 3), (4, 12)):
        nshape, ngrid, st = oracle.construct_map(shape, nodes[0]["pose"], nodes[lo:hi], alloc=alloc)
        bs = 1 << log2_block
        r0, c0 = st["row_min"], st["col_min"]
        want = oracle.derived_alloc(ngrid, log2_block)
        for br in range(want.shape[0]):
            for bc in range(want.shape[1]):
                obr, obc = br + r0 // bs, bc + c0 // bs
                if 0 <= obr < alloc.shape[0] and 0 <= obc < alloc.shape[1] and alloc[obr, obc]:
                    want[br, bc] = 1
        assert np.array_equal(st["alloc"], want)
        known = oracle.derived_alloc(ngrid, log2_block)
        assert not (known & ~st["alloc"]).any()                 # every known cell is allocated
        reset_but_allocated += int((st["alloc"] & ~known).sum())
        shape, grid, alloc = nshape, ngrid, st["alloc"]
    assert reset_but_allocated > 0


@pytest.mark.parametrize("log2_block", [3, 4, 5])
def test_update_only_allocation_equals_derived_rule(oracle, log2_block):
    """A map that was only ever updated (a local map grown scan by scan, resizes included): the
    tracked bitmap is the rule "a block is allocated iff it holds a known cell"."""
    from cost_edge_cases import local_map_steps
    grew = 0
    for step in local_map_steps(oracle, log2_block):
        assert np.array_equal(step["alloc"], oracle.derived_alloc(step["grid"], log2_block)), step["k"]
        grew += step["grew"]
    assert grew >= 1


@pytest.mark.parametrize("log2_block", [3, 4])
def test_frontend_rebuilds_keep_reset_blocks(oracle, log2_block):
    """The latest-map cycle: rebuilt maps keep blocks that hold no known cell any more, and the
    cost the library used to compute (16-cell blocks derived from the cells) differs from the
    reference's by far more than the tolerance in many frames (test_gpu_cost_edges.py's
    precondition)."""
    from cost_edge_cases import MARGIN, divergence, frontend_frames
    kept, diverging = 0, 0
    for fr in frontend_frames(oracle, log2_block):
        known = oracle.derived_alloc(fr["grid"], log2_block)
        assert not (known & ~fr["alloc"]).any()
        kept += int((fr["alloc"] & ~known).sum())
        diverging += divergence(oracle, fr["grid"], fr["query"], fr["alloc"], log2_block) > MARGIN
    assert kept > 0
    assert diverging >= 5, diverging


@pytest.mark.parametrize("log2_block", [2, 3, 4, 5])
def test_fresh_construct_divergence(oracle, log2_block):
    """Fresh constructs: the tracked bitmap is the derived rule on the map's own blocks; on
    blocks other than 16 cells the cost differs from the 16-cell rule (the B.3(a) precondition),
    on 16-cell blocks it is the same bitmap (the control)."""
    from cost_edge_cases import MARGIN, divergence, fresh_construct
    w = fresh_construct(oracle, log2_block)
    assert np.array_equal(w["alloc"], oracle.derived_alloc(w["grid"], log2_block))
    if log2_block == 4:
        assert np.array_equal(w["alloc"], oracle.derived_alloc(w["grid"], 4))
        return
    n = sum(divergence(oracle, w["grid"], q, w["alloc"], log2_block) > MARGIN for q in w["queries"])
    assert n >= 2, n


def test_local_map_divergence_off_16_cell_blocks(oracle):
    """A local map on 8-cell blocks grown by updates: the 16-cell rule reads it differently (the
    B.3(c) precondition)."""
    from cost_edge_cases import MARGIN, divergence, local_map_steps
    n = sum(divergence(oracle, s["grid"], s["query"], s["alloc"], 3) > MARGIN
            for s in local_map_steps(oracle, 3) if s["query"] is not None)
    assert n >= 2, n


def test_linear_solver_trace(oracle):
    """The oracle's per-iteration trace: one entry per iteration, each step starts from the cost
    the previous one ended with, and the damping factor follows the halving / doubling rule."""
    c = synth.csm_case(3100, n_beams=1080, fov=1.5 * math.pi)
    init = tuple(np.asarray(c["truth"]) + (0.3, -0.25, 0.05))
    w = oracle.linear_solver(c["grid"], c["geom"], c["angles"], c["ranges"], c["rel_pose"], init, 10, 1e-4,
                             1e-4, 1e4, trace=True)
    tr = w["trace"]
    assert len(tr) == w["iterations"] >= 2
    assert tr[0][0] == w["normalized_initial_cost"] * len(c["angles"])
    assert tr[-1][1] == w["normalized_cost"] * len(c["angles"])
    for (p0, c0, l0), (p1, c1, l1) in zip(tr, tr[1:]):
        assert p1 == c0
        assert l1 == (max(1e-8, l0 * 0.5) if c0 < p0 else min(1e-4, l0 * 2.0))
    plain = oracle.linear_solver(c["grid"], c["geom"], c["angles"], c["ranges"], c["rel_pose"], init, 10, 1e-4,
                                 1e-4, 1e4)
    assert plain["best_sensor_pose"] == w["best_sensor_pose"] and "trace" not in plain
