"""Crafted inputs of the three map builders (csm_construct_map_from_scans, csm_construct_maps_from_scans,
csm_construct_global_map) whose cell values depend on the ORDER of a cell's hits and misses, with the exact
sequence of every touched cell from Python. The room cases of the other map suites cannot see a hit ranked
wrongly: at the default probabilities the updates nearly commute. Here a build runs with prob_hit = 0.52 and
prob_miss = 0.1: a block of BLOCK misses takes any value to the floor 1, and from 1 every further hit gives
a new value for MAX_TAIL hits (one more reaches 65535, where longer tails run together). A target cell takes
k hits, the block, then n - k hits, so its final value names k. tests/test_cpu_map_rank_cases.py proves all
of this (the floor and the step count are recomputed there); tests/test_gpu_map_rank.py runs the cases.

Geometry as tests/ray_check_reference.py: res = 0.25, the frame before the build at offset 0, every sensor
and every beam end at the CENTRE of a sub-pixel, given as integer sub-pixel coordinates (X + 0.5) / scale
cells. No beam end lies within a rounding of a cell or sub-pixel edge, so every projection is certified on
the device. A target T lies on a ring around its sensor; its n hit beams end in T, and the BLOCK beams of
its miss block end BEYOND cells behind it in a cell U and cross T. Ray order is node order, then beam
order."""
import math

import numpy as np

import global_map_cases as GM
from oracle import oracle as O

RES = 0.25
SHAPE0 = dict(res=RES, off_x=0.0, off_y=0.0, rows=16, cols=16, log2_block=4)
PROB_HIT, PROB_MISS = 0.52, 0.1
BLOCK = 7                    # misses of a block; proven to reach the floor from any value
BEYOND = 6                   # cells from T to the block's end cell U
MAX_TAIL = 175               # the largest n - k of any target; proven to give distinct values
USABLE_MAX = 50.0
SETTINGS = dict(usable_range_min=0.01, usable_range_max=USABLE_MAX, prob_hit=PROB_HIT, prob_miss=PROB_MISS)

# where in a target cell its hit beams end, as fractions of the cell, in turn
AIMS = ((0.50, 0.50), (0.23, 0.71), (0.77, 0.31), (0.41, 0.13), (0.62, 0.88))


def build_kw(case):
    """The builder settings of a case as the api's keyword arguments."""
    return dict(SETTINGS, subpixel_scale=case["subpixel_scale"])


def oracle_kw(case):
    return dict(usable_min=SETTINGS["usable_range_min"], usable_max=USABLE_MAX, prob_hit=PROB_HIT,
                prob_miss=PROB_MISS, subpixel=case["subpixel_scale"])


# ---- construction ----

def _position(sub, scale):
    """The map-local position of the centre of sub-pixel `sub` (integers, in the frame at offset 0)."""
    return ((sub[0] + 0.5) / scale * RES, (sub[1] + 0.5) / scale * RES)


def _sub(cell, frac, scale):
    return (cell[0] * scale + int(frac[0] * scale), cell[1] * scale + int(frac[1] * scale))


def _node(sensor_sub, end_subs, scale, theta=0.0):
    """One scan node at the centre of sub-pixel sensor_sub, heading theta, its beams ending at the
    centres of the sub-pixels end_subs ([n, 2] integers), in that order."""
    sx, sy = _position(sensor_sub, scale)
    ends = np.asarray(end_subs, np.int64).reshape(-1, 2)
    dx = (ends[:, 0] + 0.5) / scale * RES - sx
    dy = (ends[:, 1] + 0.5) / scale * RES - sy
    return dict(pose=(sx, sy, theta), angles=np.arctan2(dy, dx) - theta, ranges=np.hypot(dx, dy),
                rel_pose=(0.0, 0.0, 0.0), min_range=0.0, max_range=1e9)


def _ring_target(sensor_sub, radius, phi, scale):
    """(T, the sub-pixel in U where the miss block ends) for the ring position at angle phi."""
    cx, cy = (sensor_sub[0] + 0.5) / scale, (sensor_sub[1] + 0.5) / scale
    T = (int(math.floor(cx + radius * math.cos(phi))), int(math.floor(cy + radius * math.sin(phi))))
    tx, ty = T[0] + 0.5, T[1] + 0.5
    d = math.hypot(tx - cx, ty - cy)
    f = (d + BEYOND) / d
    ux, uy = cx + f * (tx - cx), cy + f * (ty - cy)
    return T, (int(math.floor(ux * scale)), int(math.floor(uy * scale)))


def _hit_subs(T, n, scale):
    aims = np.array([_sub(T, a, scale) for a in AIMS], np.int64)
    return aims[np.arange(n) % len(AIMS)]


def _block_subs(U_sub):
    return np.tile(np.asarray(U_sub, np.int64), (BLOCK, 1))


def _ring_node(sensor_cell, frac, radius, specs, scale, slots=None, phase=0.0, theta=0.0):
    """A node whose beams are, target after target: k hits, the miss block, n - k hits (specs =
    [(n, k)], k = None: no block). Returns (node, targets)."""
    S = _sub(sensor_cell, frac, scale)
    slots = slots or len(specs)
    ends, targets = [], []
    for i, (n, k) in enumerate(specs):
        T, U_sub = _ring_target(S, radius, phase + 2.0 * math.pi * i / slots, scale)
        hits = _hit_subs(T, n, scale)
        if k is None:
            ends.append(hits)
        else:
            ends += [hits[:k], _block_subs(U_sub), hits[k:]]
        targets.append((T, n, k))
    return _node(S, np.concatenate(ends), scale, theta), targets


def _case(name, nodes, targets, scale=100, **more):
    return dict(name=name, nodes=nodes, map_pose=(0.0, 0.0, 0.0), shape=dict(SHAPE0), targets=targets,
                prob_hit=PROB_HIT, prob_miss=PROB_MISS, subpixel_scale=scale, **more)


# ---- the families ----

SWEEP_MAX_N = 50
SWEEP_BUILDS = 6
_SWEEP_CENTRES = ((0, 0), (80, 0), (0, 80), (80, 80))       # rings of radius 30 + BEYOND: they stay apart
_SWEEP_FRACS = ((0.37, 0.61), (0.12, 0.93), (0.81, 0.26), (0.55, 0.08))


def sweep():
    """Every n in 1 .. 50 with every k in 0 .. n: 1325 targets over 6 builds of 4 nodes each, dealt out
    in turn so that every ring holds small and large n."""
    specs = [(n, k) for n in range(1, SWEEP_MAX_N + 1) for k in range(n + 1)]
    rings = SWEEP_BUILDS * len(_SWEEP_CENTRES)
    slots = -(-len(specs) // rings)
    cases = []
    for b in range(SWEEP_BUILDS):
        nodes, targets = [], []
        for j, (centre, frac) in enumerate(zip(_SWEEP_CENTRES, _SWEEP_FRACS)):
            ring = j * SWEEP_BUILDS + b
            nd, tg = _ring_node(centre, frac, 30.0, specs[ring::rings], 100, slots=slots, phase=0.05 + 0.01 * ring)
            nodes.append(nd)
            targets += tg
        cases.append(_case("sweep_%d" % b, nodes, targets))
    return cases


def _tail_specs(counts, tails):
    return [(n, max(n - t, 0)) for n in counts for t in tails]


BOUNDARY_COUNTS = (32, 33, 4095, 4096, 4097)


def boundaries_default():
    """The default settings' two splits, 32 | 33 and 4096 | 4097, with the block after the last hit, before
    it, and 100 hits before the end (for 32 and 33 hits: before the first hit)."""
    nd, tg = _ring_node((0, 0), (0.37, 0.61), 14.0, _tail_specs(BOUNDARY_COUNTS, (0, 1, 100)), 100, phase=0.1)
    return _case("boundaries_default", [nd], tg, rank=(32, 4096))


LARGEST_TILE = 16384


def largest_tile():
    """One full tile of the largest size (64 KB of dynamic LDS) and one tile plus an entry."""
    specs = [(LARGEST_TILE, LARGEST_TILE - 100), (LARGEST_TILE, LARGEST_TILE), (LARGEST_TILE + 1, LARGEST_TILE),
             (LARGEST_TILE + 1, LARGEST_TILE + 1 - MAX_TAIL), (100, 50)]
    nd, tg = _ring_node((0, 0), (0.37, 0.61), 12.0, specs, 100, phase=0.2)
    return _case("largest_tile", [nd], tg, rank=(32, LARGEST_TILE))


ALL_PAIRS_CELLS = 150


def all_pairs():
    """Every beam usable, every hit cell with exactly two hits: under rank_direct_max = 1 every hit cell is
    a long cell and the two lists in hit_cells fill its rays' words exactly."""
    nd, tg = _ring_node((0, 0), (0.37, 0.61), 60.0, [(2, None)] * ALL_PAIRS_CELLS, 100, phase=0.013)
    return _case("all_pairs", [nd], tg, rank=(1, 64))


TWO_NODES_SPECS = ((1, 0), (1, 1), (2, 1), (3, 1), (3, 2), (4, 2), (5, 4), (8, 3), (9, 8), (16, 16), (17, 0),
                   (17, 9), (33, 20), (40, 7), (64, 32), (65, 33))
_TWO_NODES_SENSORS = (((0, 0), (0.37, 0.61), 0.3), ((4, -3), (0.12, 0.93), -0.5), ((-3, 2), (0.81, 0.26), 1.1))
_TWO_NODES_FRAME = 55


def two_nodes():
    """A target's first k hits come from node 0, its miss block from node 1, its other n - k hits from
    node 2, the three at different poses. Node 0 also has four beams to the corners of a frame that
    holds everything, so that a build from node 0 alone leaves the frame of the whole case."""
    scale, radius, slots = 100, 40.0, len(TWO_NODES_SPECS)
    phase = math.pi / slots
    ends = [[], [], []]
    targets = []
    centre = _sub((0, 0), (0.5, 0.5), scale)
    sensors = [_sub(cell, frac, scale) for cell, frac, _ in _TWO_NODES_SENSORS]
    for i, (n, k) in enumerate(TWO_NODES_SPECS):
        T, _ = _ring_target(centre, radius, phase + 2.0 * math.pi * i / slots, scale)
        # the block's end: BEYOND cells behind T as node 1 sees it
        bx, by = (sensors[1][0] + 0.5) / scale, (sensors[1][1] + 0.5) / scale
        d = math.hypot(T[0] + 0.5 - bx, T[1] + 0.5 - by)
        f = (d + BEYOND) / d
        U_sub = (int(math.floor((bx + f * (T[0] + 0.5 - bx)) * scale)), int(math.floor((by + f * (T[1] + 0.5 - by)) * scale)))
        hits = _hit_subs(T, n, scale)
        ends[0].append(hits[:k])
        ends[1].append(_block_subs(U_sub))
        ends[2].append(hits[k:])
        targets.append((T, n, k))
    c = _TWO_NODES_FRAME
    ends[0].append(np.array([_sub(cell, (0.31, 0.47), scale) for cell in ((c, c), (-c, c), (-c, -c), (c, -c))], np.int64))
    nodes = [_node(sensors[j], np.concatenate(ends[j]), scale, _TWO_NODES_SENSORS[j][2]) for j in range(3)]
    return _case("two_nodes", nodes, targets)


def walks(scale):
    """The exact walks of ray_check_reference.named_cases() as beams of a map build, every end at a
    sub-pixel centre: vertical both ways, horizontal both ways, rising and falling through exact cell
    corners, steep rays of two columns with more than 64 cells, shallow rays over more than 64 columns,
    beams whose end lies left of the sensor. Six nodes, one sensor each."""
    s = scale
    h = s // 2
    nodes = []

    def add(S, ends):
        nodes.append(_node(S, [(S[0] + dx, S[1] + dy) for dx, dy in ends], scale))

    # one column (the same sub-pixel column, and another one of the same cell), one row
    add(_sub((40, 30), (0.37, 0.61), s), [(0, 48 * s), (0, -20 * s), (int(0.4 * s), 9 * s), (24 * s, 0), (-28 * s, 0)])
    # exact corners: equal fractions in x and y (rising); fractions that add up to one cell (falling)
    add((40 * s + h, 30 * s + h), [(12 * s, 12 * s), (-11 * s, -11 * s)])
    add((40 * s + h, 30 * s + s - 1 - h), [(9 * s, -9 * s), (-7 * s, 7 * s)])
    # two columns, more than 64 rows
    step = max(1, int(0.6 * s))
    add(_sub((15, 5), (0.7, 0.3), s), [(step, 70 * s), (step, -3 * s), (-step - int(0.7 * s), 66 * s)])
    # more than 64 columns: rising, falling, and a short one to the left
    add(_sub((8, 10), (0.4, 0.55), s), [(80 * s + int(0.13 * s), 2 * s), (70 * s, -3 * s), (-6 * s, s // 3)])
    # the end left of the sensor
    add(_sub((40, 30), (0.3, 0.45), s), [(-27 * s, 8 * s + 3), (-24 * s, -10 * s - 1), (-1 - int(0.2 * s), 5 * s)])
    return _case("walks_%d" % scale, nodes, [], scale=scale)


WALK_SCALES = (1, 100)

# name -> maker of a list of cases
FAMILIES = {
    "sweep": sweep,
    "boundaries_default": lambda: [boundaries_default()],
    "largest_tile": lambda: [largest_tile()],
    "all_pairs": lambda: [all_pairs()],
    "two_nodes": lambda: [two_nodes()],
    "walks": lambda: [walks(s) for s in WALK_SCALES],
}


def build(families=None):
    """[(name, case)] of the named families (all of them: None), in the table's order."""
    return [(c["name"], c) for f, make in FAMILIES.items() if families is None or f in families for c in make()]


# ---- the reference: every touched cell's sequence of hits and misses ----

def rays_of(case, shape):
    """Every usable ray in order (node order, then beam order), in the frame `shape` (the frame after the
    build): dict(node, s, e, H, cells) with the sub-pixel start and end, the hit cell and the cells of
    oracle.ray_cells with the end cell removed as the builder removes it (the first entry equal to it)."""
    res, off_x, off_y = shape["res"], shape["off_x"], shape["off_y"]
    scale = case["subpixel_scale"]
    scaled = res / scale
    walked = {}
    out = []
    for k, nd in enumerate(case["nodes"]):
        ls = O.inverse_compound(case["map_pose"], O.compound(nd["pose"], nd.get("rel_pose", (0.0, 0.0, 0.0))))
        lx, ly, lt = float(ls[0]), float(ls[1]), float(ls[2])
        sx, sy = int(math.floor((lx - off_x) / scaled)), int(math.floor((ly - off_y) / scaled))
        lo = max(SETTINGS["usable_range_min"], nd.get("min_range", 0.0))
        hi = min(USABLE_MAX, nd.get("max_range", 1e9))
        for a, r in zip(np.asarray(nd["angles"], np.float64).tolist(), np.asarray(nd["ranges"], np.float64).tolist()):
            if r >= hi or r <= lo:
                continue
            hx, hy = lx + r * math.cos(lt + a), ly + r * math.sin(lt + a)
            H = (int(math.floor((hx - off_x) / res)), int(math.floor((hy - off_y) / res)))
            ex, ey = int(math.floor((hx - off_x) / scaled)), int(math.floor((hy - off_y) / scaled))
            key = (sx, sy, ex, ey)
            if key not in walked:
                cells = [(int(x), int(y)) for x, y in O.ray_cells(sx, sy, ex, ey, scale, cap=1 << 10)]
                end = (ex // scale, ey // scale)
                if end in cells:
                    cells.remove(end)
                walked[key] = cells
            out.append(dict(node=k, s=(sx, sy), e=(ex, ey), H=H, cells=walked[key]))
    return out


def cell_sequences(case, shape):
    """{(col, row): its updates in order, one letter each: "M" a miss, "H" a hit}."""
    seq = {}
    for ray in rays_of(case, shape):
        for c in ray["cells"]:
            seq.setdefault(c, []).append("M")
        seq.setdefault(ray["H"], []).append("H")
    return {c: "".join(s) for c, s in seq.items()}


_TABLES = {}


def update_tables(prob_hit, prob_miss):
    """(hit, miss): value -> value after one update, for every value, from oracle.bayes_update."""
    key = (prob_hit, prob_miss)
    if key not in _TABLES:
        _TABLES[key] = tuple(np.array([O.bayes_update(v, p) for v in range(65536)], np.int64) for p in key)
    return _TABLES[key]


def value_of(seq, prob_hit=PROB_HIT, prob_miss=PROB_MISS):
    """The value a cell ends with after the updates `seq`, starting from 0 (unknown)."""
    v = 0
    for letter in seq:
        v = O.bayes_update(v, prob_hit if letter == "H" else prob_miss)
    return v


def planned(n, k):
    """A target's sequence: k hits, the miss block, n - k hits (k = None: no block)."""
    return "H" * n if k is None else "H" * k + "M" * BLOCK + "H" * (n - k)


def values_by_block_position(n, prob_hit=PROB_HIT, prob_miss=PROB_MISS):
    """[n + 1] the value of planned(n, k) for every k, through the tables (all positions at once)."""
    hit, miss = update_tables(prob_hit, prob_miss)
    v = np.zeros(n + 1, np.int64)
    for k in range(1, n + 1):            # entry k takes k hits
        v[k:] = hit[v[k:]]
    for _ in range(BLOCK):
        v = miss[v]
    for j in range(1, n + 1):            # entry k takes n - k more
        v[:n - j + 1] = hit[v[:n - j + 1]]
    return v


def in_frame(cell, shape):
    """A cell given in the frame at offset 0, as (col, row) of the frame `shape`."""
    return (cell[0] - int(round(shape["off_x"] / shape["res"])), cell[1] - int(round(shape["off_y"] / shape["res"])))


_COUNTS = {}


def hit_counts(case, shape, nodes=None):
    """The number of hits of every cell with hits (sorted), from the nodes `nodes` alone (all: None)."""
    key = (case["name"], shape["off_x"], shape["off_y"], None if nodes is None else tuple(nodes))
    if key not in _COUNTS:
        part = case if nodes is None else dict(case, nodes=[case["nodes"][k] for k in nodes])
        counts = {}
        for ray in rays_of(part, shape):
            counts[ray["H"]] = counts.get(ray["H"], 0) + 1
        _COUNTS[key] = np.sort(np.array(list(counts.values()), np.int64))
        _COUNTS[key].setflags(write=False)
    return _COUNTS[key]


def rank_info(case, shape, rank, parts=None):
    """What csm_global_map_info reports for the case under a rank setting: the hit cells per rank path and
    the largest hit count, the cells counted part by part (parts = lists of node numbers; None: one)."""
    out = dict(direct_cells=0, sorted_cells=0, tiled_cells=0, max_hits_per_cell=0)
    for nodes in (parts or [None]):
        counts = hit_counts(case, shape, nodes)
        taken = GM.paths_taken(counts, rank)
        for path in ("direct", "sorted", "tiled"):
            out[path + "_cells"] += taken[path]
        out["max_hits_per_cell"] = max(out["max_hits_per_cell"], int(counts.max()) if counts.size else 0)
    return out
