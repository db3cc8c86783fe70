"""The free-space check of loop candidates (include/csm_hip.h, csm_ray_check_batch) in numpy: the contract
every other layer equals. Poses come from api.host_compound, hit points from the same double expressions,
the cells of a ray from oracle.ray_cells (the step-by-step BresenhamScaled) after the whole-cell move that
makes the coordinates non-negative. Also the named cases of tests/test_cpu_ray_check.py and
tests/test_gpu_ray_check.py: hand-made grids of at most 96 x 80 cells, each with what it aims at."""
import math

import numpy as np

from csm_hip import api
from oracle import oracle as O

FIELDS = ("beams", "usable", "walked", "blocked", "end_inside", "end_occupied", "end_free", "end_unknown",
          "cells", "cells_free", "cells_unknown", "cells_near", "cells_blocking", "max_depth")   # host_beams aside

WALL, FREE, OTHER = 60000, 3000, 20000
PARAMS = dict(usable_range_min=0.01, usable_range_max=20.0, subpixel_scale=100, occupied_min=40000, free_max=10000,
              end_tolerance=1)


def params(**kw):
    p = dict(PARAMS)
    p.update(kw)
    return p


def strip(record):
    return {k: record[k] for k in FIELDS}


def beam_walks(geom, angles, ranges, rel_pose, pose, prm):
    """Per beam None (unusable) or dict(s, e, H, cells): the sub-pixel start and end, the hit cell and the
    cells W of the ray (E still in it), in map cells."""
    res, off_x, off_y = geom
    scale = prm["subpixel_scale"]
    S = api.host_compound(pose, rel_pose)
    scaled = res / scale
    sx, sy = int(math.floor((S[0] - off_x) / scaled)), int(math.floor((S[1] - off_y) / scaled))
    out = []
    for a, r in zip(np.asarray(angles, np.float64).tolist(), np.asarray(ranges, np.float64).tolist()):
        if not (r > prm["usable_range_min"] and r < prm["usable_range_max"]):
            out.append(None)
            continue
        hx = S[0] + r * math.cos(S[2] + a)
        hy = S[1] + r * math.sin(S[2] + a)
        H = (int(math.floor((hx - off_x) / res)), int(math.floor((hy - off_y) / res)))
        ex, ey = int(math.floor((hx - off_x) / scaled)), int(math.floor((hy - off_y) / scaled))
        bx, by = min(sx, ex) // scale, min(sy, ey) // scale          # Python's // is floored
        cells = O.ray_cells(sx - bx * scale, sy - by * scale, ex - bx * scale, ey - by * scale, scale)
        out.append(dict(s=(sx, sy), e=(ex, ey), H=H, cells=[(int(x) + bx, int(y) + by) for x, y in cells]))
    return out


def ray_check(grid, geom, angles, ranges, rel_pose, pose, prm):
    """(record dict without host_beams, int32 words per beam)."""
    g = np.asarray(grid)
    rows, cols = g.shape
    scale, tol = prm["subpixel_scale"], prm["end_tolerance"]
    rec = dict.fromkeys(FIELDS, 0)
    rec["beams"] = len(angles)
    words = np.zeros(len(angles), np.int32)
    for i, w in enumerate(beam_walks(geom, angles, ranges, rel_pose, pose, prm)):
        if w is None:
            words[i] = -2
            continue
        rec["usable"] += 1
        E = (w["e"][0] // scale, w["e"][1] // scale)
        missed = list(w["cells"])
        if E in missed:
            missed.remove(E)
        H = w["H"]
        any_cell, depth = False, 0
        for (x, y) in missed:
            if not (0 <= x < cols and 0 <= y < rows):
                continue
            any_cell = True
            v = int(g[y, x])
            rec["cells"] += 1
            if v == 0:
                rec["cells_unknown"] += 1
            elif v <= prm["free_max"]:
                rec["cells_free"] += 1
            elif v >= prm["occupied_min"]:
                d = max(abs(x - H[0]), abs(y - H[1]))
                if d > tol:
                    rec["cells_blocking"] += 1
                    depth = max(depth, d)
                else:
                    rec["cells_near"] += 1
        end_in = 0 <= H[0] < cols and 0 <= H[1] < rows
        if end_in:
            v = int(g[H[1], H[0]])
            rec["end_inside"] += 1
            rec["end_unknown"] += v == 0
            rec["end_free"] += 0 < v <= prm["free_max"]
            rec["end_occupied"] += v >= prm["occupied_min"]
        words[i] = -1
        if any_cell or end_in:
            rec["walked"] += 1
            words[i] = depth
            rec["blocked"] += depth > 0
            rec["max_depth"] = max(rec["max_depth"], depth)
    return {k: int(v) for k, v in rec.items()}, words


def check_case(case):
    return ray_check(case["grid"], case["geom"], case["angles"], case["ranges"], case["rel_pose"], case["pose"],
                     case["params"])


def check_passes(record, max_blocked_rate, min_walked, min_end_occupied_rate):
    """The keep rule of the C++ adapters' DetectChecked."""
    return (record["walked"] >= min_walked and record["blocked"] <= max_blocked_rate * record["walked"]
            and record["end_occupied"] >= min_end_occupied_rate * record["end_inside"])


# ---- named cases ----

def room(rows, cols, rim=4, wall=2):
    """An unknown rim, a wall band of WALL, an interior of FREE, a few cells of OTHER."""
    g = np.zeros((rows, cols), np.uint16)
    g[rim:rows - rim, rim:cols - rim] = WALL
    g[rim + wall:rows - rim - wall, rim + wall:cols - rim - wall] = FREE
    for k in range(3):
        r, c = rim + wall + 2 + 5 * k, rim + wall + 3 + 7 * k
        if r < rows - rim - wall and c < cols - rim - wall:
            g[r, c] = OTHER
    return g


RES = 0.25           # a power of two with offsets that are multiples of it: every coordinate below is exact
GEOM = (RES, -2.0, -1.0)


def _at(col, row, geom=GEOM):
    """The map-local position of cell (col, row)'s centre."""
    return (geom[1] + (col + 0.5) * geom[0], geom[2] + (row + 0.5) * geom[0])


def _case(name, grid, angles, ranges, pose, aims, walk=None, geom=GEOM, rel_pose=(0.0, 0.0, 0.0), **prm):
    return dict(name=name, grid=np.ascontiguousarray(grid, np.uint16), geom=geom,
                angles=np.asarray(angles, np.float64), ranges=np.asarray(ranges, np.float64), rel_pose=rel_pose,
                pose=tuple(pose), params=params(**prm), aims=aims, walk=walk)


def _fan(n, r_lo=1.0, r_hi=9.0, seed=0):
    rng = np.random.RandomState(seed)
    return -math.pi + 2 * math.pi * np.arange(n) / n, r_lo + (r_hi - r_lo) * rng.rand(n)


def _walk_has(pred):
    return lambda walks: any(w is not None and pred(w) for w in walks)


def _columns(w):
    return len({x for x, _ in w["cells"]})


def _diagonal(w):
    c = w["cells"]
    return any(a[0] != b[0] and a[1] != b[1] for a, b in zip(c, c[1:]))


def named_cases():
    cases = []
    g = room(80, 96)
    cx, cy = _at(40, 30)
    half = math.pi / 2
    # exact walks
    cases.append(_case("vertical_up_down", g, [half, -half], [12.1, 5.0], (cx, cy, 0.0),
                       lambda r: r["walked"] == 2 and r["cells_free"] > 0 and r["blocked"] > 0,
                       _walk_has(lambda w: _columns(w) == 1 and len(w["cells"]) > 8)))
    cases.append(_case("horizontal", g, [0.0, math.pi], [6.0, 7.0], (cx, cy, 0.0),
                       lambda r: r["walked"] == 2 and r["cells_free"] > 0,
                       _walk_has(lambda w: len({y for _, y in w["cells"]}) == 1 and _columns(w) > 8)))
    diag = math.sqrt(2.0) * RES
    # through exact cell corners: sub-pixel centres on a diagonal of the cells (rising: equal fractions in x
    # and y; falling: fractions that add up to one cell)
    cases.append(_case("corners_rising", g, [math.pi / 4, -3 * math.pi / 4], [12 * diag, 11 * diag],
                       (cx + 0.005 * RES, cy + 0.005 * RES, 0.0),
                       lambda r: r["walked"] == 2 and r["cells_free"] > 0,
                       lambda walks: all(w is not None and _diagonal(w) for w in walks)))
    cases.append(_case("corners_falling", g, [-math.pi / 4, 3 * math.pi / 4], [9 * diag, 7 * diag],
                       (cx + 0.005 * RES, cy - 0.005 * RES, 0.0),
                       lambda r: r["walked"] == 2 and r["cells_free"] > 0,
                       lambda walks: all(w is not None and _diagonal(w) for w in walks)))
    # long and steep rays
    tall = room(80, 31)
    sx, sy = _at(15, 5)
    steep = math.atan2(70.0, 0.6)
    cases.append(_case("steep_column_pair", tall, [steep, -steep + 0.0], [70.1 * RES, 3 * RES], (sx, sy, 0.0),
                       lambda r: r["walked"] == 2 and r["cells_blocking"] > 0 and r["cells_unknown"] > 0,
                       _walk_has(lambda w: _columns(w) == 2 and len(w["cells"]) > 64)))
    wide = room(21, 96)
    wx, wy = _at(8, 10)
    cases.append(_case("more_than_64_columns", wide, [0.02, math.pi - 0.03], [80 * RES, 6 * RES], (wx, wy, 0.0),
                       lambda r: r["walked"] == 2 and r["cells_free"] > 64 and r["blocked"] == 1,
                       _walk_has(lambda w: _columns(w) > 64), usable_range_max=30.0))
    cases.append(_case("start_right_of_end", g, [math.pi - 0.3, math.pi + 0.4], [7.0, 6.5], (cx, cy, 0.0),
                       lambda r: r["walked"] == 2 and r["cells_free"] > 0,
                       lambda walks: all(w is not None and w["s"][0] > w["e"][0] for w in walks)))
    # edges of the map
    a, r = _fan(24, 3.0, 9.0, seed=1)
    ox, oy = _at(-9, -7)
    cases.append(_case("sensor_outside_low", g, a, r, (ox, oy, 0.3),
                       lambda r: r["usable"] > r["walked"] > 0 and r["cells_unknown"] > 0,
                       _walk_has(lambda w: w["s"][0] < 0 and w["s"][1] < 0)))
    ex_, ey_ = _at(40, 40)
    cases.append(_case("end_outside_four_sides", g, [0.0, half, math.pi, -half], [19.0, 15.0, 16.0, 14.0],
                       (ex_, ey_, 0.0),
                       lambda r: r["walked"] == 4 and r["end_inside"] == 0 and r["blocked"] == 4 and r["cells_near"] == 0))
    fx, fy = _at(150, 120)
    cases.append(_case("wholly_outside", g, [0.0, 0.7, half], [3.0, 4.0, 5.0], (fx, fy, 0.0),
                       lambda r: r["usable"] == 3 and r["walked"] == 0 and r["cells"] == 0))
    cases.append(_case("sensor_and_hit_in_one_cell", g, [0.0, 2.0], [0.05, 0.07], (cx, cy, 0.0),
                       lambda r: r["walked"] == 2 and r["cells"] == 0 and r["end_free"] == 2))
    # usable range and beam count
    cases.append(_case("usable_limits_and_nan", g, np.linspace(-1.0, 1.0, 7),
                       [0.01, 0.0100001, 19.999999, 20.0, 25.0, float("nan"), 3.0], (cx, cy, 0.0),
                       lambda r: r["beams"] == 7 and r["usable"] == 3))
    for n in (1, 63, 65, 1081):
        a, r = _fan(n, 0.5, 9.5, seed=n)
        cases.append(_case("beams_%d" % n, g, a, r, (cx + 0.013, cy - 0.021, 0.1 * n),
                           lambda r, n=n: r["beams"] == n and r["usable"] == n and r["walked"] > 0))
    # parameter sweeps: a wall two cells thick, near and blocking on one ray
    odd = room(41, 67)
    px, py = _at(30, 20)
    a, r = _fan(90, 8.0 * RES, 38.0 * RES, seed=5)
    for scale in (1, 7, 100):
        for tol in (0, 1, 3):
            cases.append(_case("scale_%d_tolerance_%d" % (scale, tol), odd, a, r, (px + 0.031, py + 0.017, 0.05),
                               lambda r, tol=tol: r["blocked"] > 0 and (r["cells_near"] > 0 or tol == 0)
                               and r["cells_unknown"] > 0 and r["cells_free"] > 0 and r["end_occupied"] > 0,
                               subpixel_scale=scale, end_tolerance=tol))
    # the wall case with a sensor off the robot, on a geometry that is not exact
    cases.append(_case("wall_offset_sensor", odd, a, 0.2 * r, (0.417, 0.233, -0.4),
                       lambda r: r["blocked"] > 0 and r["cells_near"] > 0 and r["cells_unknown"] > 0
                       and r["cells"] > r["cells_free"] + r["cells_unknown"] + r["cells_near"] + r["cells_blocking"],
                       geom=(0.05, -1.5137, -0.9219), rel_pose=(0.11, -0.07, 0.3), usable_range_max=1.8,
                       usable_range_min=0.5))
    # degenerate maps
    one_row = np.full((1, 40), FREE, np.uint16)
    one_row[0, 30:32] = WALL
    rx, ry = _at(5, 0)
    cases.append(_case("one_row", one_row, [0.0, 0.001, half, -0.4], [7.0, 8.0, 2.0, 3.0], (rx, ry, 0.0),
                       lambda r: r["walked"] == 4 and r["blocked"] > 0 and r["cells_free"] > 0))
    a, r = _fan(33, 1.0, 6.0, seed=9)
    cases.append(_case("all_zeros", np.zeros((37, 45), np.uint16), a, r, _at(20, 18) + (0.0,),
                       lambda r: r["walked"] > 0 and r["cells"] == r["cells_unknown"] > 0 and r["blocked"] == 0
                       and r["end_unknown"] == r["end_inside"] > 0))
    return cases
