"""Inputs of tests/test_gpu_mixed_batch.py that the CPU suite checks too
(tests/test_cpu_mixed_batch_cases.py): one pool of maps and loop-detection queries that differ the
way the queries of one Detect() call do. Three map resolutions (so every call forms at least three
groups of one padded leaf-window extent, csm_batch.hip's loop_batch), maps of odd sizes, a long thin
one, an edge-band one, a tie-prone one, a mostly unknown one and one uploaded as blocks with some of
them unallocated; scans of 1 to 5000 beams, dense and sparse, 5 m and 20 m maximum ranges, non-zero
relative sensor poses, one query off its map; scan arrays shared within and across groups. The
queries come in interleaved order: neighbours usually belong to different groups. Pure numpy and
the host restatements of the planner's decisions; no GPU."""
import math

import numpy as np

from csm_hip import synth

RES = (0.025, 0.05, 0.1)
BLOCK_LOG2 = 4
FLAGGED = 1 | 2 | 8 | 16          # EDGE_BAND | KEY_TIE | LITERAL | PROJ_DELTA (include/csm_hip.h)


def merging_pays(angles, ranges, res):
    """csm_plan.hip's merging_pays: do enough beams share cells for the weighted (merged) entry
    lists to pay? The group's first query decides fine.weighted for the whole group."""
    n = len(angles)
    if n < 2:
        return False
    cells = 1.0
    for i in range(1, n):
        arc = abs(angles[i] - angles[i - 1]) * 0.5 * (ranges[i] + ranges[i - 1])
        cells += min(1.0, arc / res)
    return n >= 1.4 * cells


def padded_extent(win, unit):
    """csm_plan.hip's padded_extent: candidates per axis, padded to a multiple of unit."""
    return -(-(2 * win + 1) // unit) * unit


def _blocks_of(grid, allocated):
    bs = 1 << BLOCK_LOG2
    br, bc = grid.shape[0] // bs, grid.shape[1] // bs
    blocks, dense = [], grid.copy()
    for r in range(br):
        for c in range(bc):
            if allocated[r, c]:
                blocks.append(grid[r * bs:(r + 1) * bs, c * bs:(c + 1) * bs].copy())
            else:
                blocks.append(None)
                dense[r * bs:(r + 1) * bs, c * bs:(c + 1) * bs] = 0      # what an unallocated block reads
    return blocks, br, bc, dense


def _map(seed, res, rows, cols, **kw):
    grid, geom, segs = synth.make_room(seed, rows, cols, res, **kw)
    return dict(grid=grid, geom=geom, segs=segs, blocks=None)


def _scan(m, seed, n_beams, max_range=5.7296, fov=2 * math.pi, init_error=(0.11, -0.07, 0.02)):
    """A scan cast in map m's room from a seeded true pose, and the initial pose off it by init_error."""
    rng = np.random.RandomState(seed)
    truth = (0.2 * (rng.rand() - 0.5), 0.2 * (rng.rand() - 0.5), 0.1 * (rng.rand() - 0.5))
    angles, ranges = synth.cast_scan(m["segs"], truth, n_beams, fov, max_range)
    init = (truth[0] + init_error[0], truth[1] + init_error[1], truth[2] + init_error[2])
    return angles, ranges, init


def make_pool(seed=0):
    """Returns dict(maps={map_id: dict(grid (what the device sees), geom, blocks)}, queries=[...]).
    A query is dict(name, map_id, geom, angles, ranges, rel_pose, init_pose); queries that share a
    scan hold the very same numpy arrays."""
    base = 9100 + 100 * seed
    maps = {
        # res 0.025: a map of 136 x 152 cells whose room reaches its low edges (edge band)
        base + 0: _map(seed + 11, 0.025, 136, 152, origin="low_edge", n_boxes=2),
        # res 0.05: the shared map, edge band, integer-key ties, mostly unknown, long and thin, blocks
        base + 1: _map(seed + 12, 0.05, 400, 400),
        base + 2: _map(seed + 13, 0.05, 256, 288, origin="low_edge", half_x=5.2, half_y=4.4),
        base + 3: _map(seed + 14, 0.05, 200, 232, levels=3, interior_unknown=0.0),
        base + 4: _map(seed + 15, 0.05, 240, 264, interior_unknown=0.85),
        base + 5: _map(seed + 16, 0.05, 72, 520, n_boxes=3),
        base + 6: _map(seed + 17, 0.05, 400, 400),
        # res 0.1: a 40 m map and a tie-prone one
        base + 7: _map(seed + 18, 0.1, 400, 400),
        base + 8: _map(seed + 19, 0.1, 136, 152, levels=3, interior_unknown=0.0),
    }
    # the block-uploaded map: blocks that hold nothing known stay unallocated, and a few more
    g = maps[base + 6]["grid"]
    bs = 1 << BLOCK_LOG2
    known = g.reshape(g.shape[0] // bs, bs, g.shape[1] // bs, bs).max(axis=(1, 3)) > 0
    allocated = known.copy()
    allocated[3:6, 7:9] = False         # inside the room: reads 0 there
    blocks, br, bc, dense = _blocks_of(g, allocated)
    maps[base + 6].update(grid=dense, blocks=(blocks, br, bc, BLOCK_LOG2))

    q = []

    def add(name, map_id, angles, ranges, init, rel=(0.0, 0.0, 0.0)):
        q.append(dict(name=name, map_id=map_id, geom=maps[map_id]["geom"], angles=angles, ranges=ranges,
                      rel_pose=tuple(rel), init_pose=tuple(init)))

    m = maps
    # res 0.025 group: a dense scan first, a sparse one last (reversing the batch swaps them)
    a1080 = _scan(m[base + 0], seed + 21, 1080, init_error=(0.09, 0.08, 0.02))
    a360 = _scan(m[base + 0], seed + 22, 360, init_error=(0.12, 0.1, 0.03))
    a7 = _scan(m[base + 0], seed + 23, 7)
    a1 = _scan(m[base + 0], seed + 24, 1)
    # res 0.05
    s360 = _scan(m[base + 1], seed + 31, 360)                      # shared by several queries
    s5000 = _scan(m[base + 1], seed + 32, 5000, init_error=(-0.08, 0.06, -0.015))
    s20 = _scan(m[base + 1], seed + 33, 360, max_range=20.0)       # a 20 m beam: many more slices
    e360 = _scan(m[base + 2], seed + 34, 360, init_error=(0.23, 0.19, 0.03))
    t540 = _scan(m[base + 3], seed + 35, 540)
    u360 = _scan(m[base + 4], seed + 36, 360)
    n360 = _scan(m[base + 5], seed + 37, 360, fov=1.5 * math.pi)
    k720 = _scan(m[base + 6], seed + 38, 720)
    # res 0.1
    c1080 = _scan(m[base + 7], seed + 41, 1080, init_error=(0.3, -0.2, 0.02))
    c90 = _scan(m[base + 7], seed + 42, 90)
    t360 = _scan(m[base + 8], seed + 43, 360)

    rel = (0.12, -0.05, 0.03)
    groups = [
        [("a_dense", base + 0, a1080, None), ("a_rel", base + 0, a360, rel),
         ("a_shared_c", base + 0, (c90[0], c90[1], a7[2]), None), ("a_one", base + 0, a1, None),
         ("a_sparse", base + 0, a7, None)],
        [("b_5000", base + 1, s5000, None), ("b_360", base + 1, s360, None),
         ("e_edge", base + 2, e360, None), ("t_tie", base + 3, t540, None),
         ("b_long", base + 1, s20, None), ("u_unknown", base + 4, u360, None),
         ("n_thin", base + 5, n360, None), ("k_blocks", base + 6, k720, rel),
         ("b_off", base + 1, (s360[0], s360[1], (61.0, -43.0, 0.4)), None),
         ("t_shared", base + 3, (s360[0], s360[1], t540[2]), None), ("b_one", base + 1, a1, None)],
        [("c_dense", base + 7, c1080, None), ("c_shared_b", base + 7, (s360[0], s360[1], c1080[2]), None),
         ("c_tie", base + 8, t360, rel), ("c_sparse", base + 7, c90, None)],
    ]
    per_group = []
    for grp in groups:
        lst = []
        for name, mid, (angles, ranges, init), r in grp:
            lst.append((name, mid, angles, ranges, init, r or (0.0, 0.0, 0.0)))
        per_group.append(lst)
    # interleave: one query of every resolution in turn
    while any(per_group):
        for lst in per_group:
            if lst:
                name, mid, angles, ranges, init, r = lst.pop(0)
                add(name, mid, angles, ranges, init, r)
    return dict(maps=maps, queries=q)


def oracle_case(pool, query):
    """The oracle's view of a query: the map as the device holds it plus the scan and poses."""
    m = pool["maps"][query["map_id"]]
    return dict(grid=m["grid"], geom=query["geom"], angles=query["angles"], ranges=query["ranges"],
                rel_pose=query["rel_pose"], init_pose=query["init_pose"])


def long_range_subset(pool):
    """The queries of the range_theta = 2 pi call: no scan above 1080 beams, none at 0.025 m above
    seven beams (their 1441 slices of 41 x 41 candidates would make the oracle slow)."""
    keep = []
    for q in pool["queries"]:
        n, res = len(q["angles"]), q["geom"][0]
        if n > 1080 or (res < 0.04 and n > 7) or (res > 0.07 and n > 360):
            continue
        keep.append(q)
    return keep


def group_key(query, host_search_step, host_window, range_x, range_y, unit):
    """loop_batch's group key of a query: the padded leaf-window extents."""
    sx, sy, _ = host_search_step(query["geom"][0], query["ranges"])
    return (padded_extent(host_window(range_x, sx), unit), padded_extent(host_window(range_y, sy), unit))


def n_theta(query, host_search_step, host_window, range_theta):
    _, _, st = host_search_step(query["geom"][0], query["ranges"])
    return 2 * host_window(range_theta, st) + 1


def groups_in_order(queries, key_of):
    """{key: [input indices]} in input order, as loop_batch builds them."""
    out = {}
    for i, q in enumerate(queries):
        out.setdefault(key_of(q), []).append(i)
    return out
