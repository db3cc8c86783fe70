"""The free-space check of loop candidates (include/csm_hip.h, csm_ray_check_batch) in numpy: the contract
every other layer equals. Poses come from api.host_compound, hit points from the same double expressions,
the cells of a ray from oracle.ray_cells (the step-by-step BresenhamScaled) after the whole-cell move that
makes the coordinates non-negative. Also the named cases of tests/test_cpu_ray_check.py and
tests/test_gpu_ray_check.py: hand-made grids of at most 96 x 80 cells, each with what it aims at.

For the edge suites (tests/test_cpu_ray_check_edges.py, tests/test_gpu_ray_check_edges.py): window_cells, the
cells of a walk inside a window from Python integers alone, and ray_check_windowed on top of it, which far
frames need (a ray of 2^20 cells is too long for the step-by-step walk); far_cases, clip_cases,
threshold_cases, the bookkeeping cases and sweep_cases."""
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


# ---- the same definition in unbounded integers, restricted to a window ----

def window_cells(sx, sy, ex, ey, scale, c_lo, c_hi, r_lo, r_hi):
    """The cells (x, y) of the walk from (sx, sy) to (ex, ey) (non-negative sub-pixel coordinates) with
    c_lo <= x <= c_hi and r_lo <= y <= r_hi, column after column. Python ints only: nothing overflows, and
    the columns and rows outside the window cost nothing. The ray's height at cell edge x = c, counted in
    1 / den cells, is N(c); column c holds the rows from where the ray enters it to where it leaves it, and
    a ray that leaves through an exact corner steps diagonally."""
    sx, sy, ex, ey, scale = int(sx), int(sy), int(ex), int(ey), int(scale)
    if sx > ex:
        sx, sy, ex, ey = ex, ey, sx, sy
    x0, y0, x1, y1 = sx // scale, sy // scale, ex // scale, ey // scale
    out = []
    if x0 == x1:
        if c_lo <= x0 <= c_hi:
            out += [(x0, y) for y in range(max(min(y0, y1), r_lo), min(max(y0, y1), r_hi) + 1)]
        return out
    dx, dy = ex - sx, ey - sy
    den = 2 * scale * dx
    ns = (2 * sy + 1) * dx
    ne = ns + 2 * dy * dx

    def height(c):
        return ns + dy * (2 * scale * c - (2 * sx + 1))

    for c in range(max(x0, c_lo), min(x1, c_hi) + 1):
        a = ns if c == x0 else height(c)
        b = ne if c == x1 else height(c + 1)
        if dy > 0:
            lo, hi = (y0 if c == x0 else a // den), -(-b // den) - 1
        else:
            lo, hi = b // den, (y0 if c == x0 else -(-a // den) - 1)
        out += [(c, y) for y in range(max(lo, r_lo), min(hi, r_hi) + 1)]
    return out


def beam_ends(geom, angles, ranges, rel_pose, pose, prm):
    """beam_walks without the cells: per beam None (unusable) or dict(s, e, H)."""
    res, off_x, off_y = geom
    S = api.host_compound(pose, rel_pose)
    scaled = res / prm["subpixel_scale"]
    s = (int(math.floor((S[0] - off_x) / scaled)), int(math.floor((S[1] - off_y) / scaled)))
    out = []
    for a, r in zip(np.asarray(angles, np.float64).tolist(), np.asarray(ranges, np.float64).tolist()):
        if not (r > prm["usable_range_min"] and r < prm["usable_range_max"]):
            out.append(None)
            continue
        hx = S[0] + r * math.cos(S[2] + a)
        hy = S[1] + r * math.sin(S[2] + a)
        out.append(dict(s=s, e=(int(math.floor((hx - off_x) / scaled)), int(math.floor((hy - off_y) / scaled))),
                        H=(int(math.floor((hx - off_x) / res)), int(math.floor((hy - off_y) / res)))))
    return out


def largest_product(w, scale):
    """The largest n0 + |dy| (first + 2 scale m) of the closed form (csm_map.hpp) for the beam w of beam_ends,
    after the whole-cell move; 0 for a one-column ray, which takes no product."""
    (sx, sy), (ex, ey) = w["s"], w["e"]
    bx, by = min(sx, ex) // scale, min(sy, ey) // scale
    sx, sy, ex, ey = sx - bx * scale, sy - by * scale, ex - bx * scale, ey - by * scale
    if sx > ex:
        sx, sy, ex, ey = ex, ey, sx, sy
    m = ex // scale - sx // scale
    if m == 0:
        return 0
    dx, dy = ex - sx, ey - sy
    n0 = (sy // scale) * 2 * scale * dx + (2 * (sy % scale) + 1) * dx
    first = 2 * scale - (2 * (sx % scale) + 1)
    return n0 + abs(dy) * (first + 2 * scale * m)


def ray_check_windowed(grid, geom, angles, ranges, rel_pose, pose, prm):
    """ray_check with the missed cells from window_cells over the map's own rectangle: what it costs depends
    on the map, not on the length of the rays."""
    g = np.asarray(grid)
    rows, cols = g.shape
    scale, tol = prm["subpixel_scale"], prm["end_tolerance"]
    rec = dict.fromkeys(FIELDS, 0)
    rec["beams"] = len(angles)
    words = np.zeros(len(angles), np.int32)
    for i, w in enumerate(beam_ends(geom, angles, ranges, rel_pose, pose, prm)):
        if w is None:
            words[i] = -2
            continue
        rec["usable"] += 1
        (sx, sy), (ex, ey), H = w["s"], w["e"], w["H"]
        E = (ex // scale, ey // scale)
        bx, by = min(sx, ex) // scale, min(sy, ey) // scale
        inside = window_cells(sx - bx * scale, sy - by * scale, ex - bx * scale, ey - by * scale, scale,
                              -bx, cols - 1 - bx, -by, rows - 1 - by)
        any_cell, depth = False, 0
        for (x, y) in ((x + bx, y + by) for x, y in inside):
            if (x, y) == E:
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


def check_case_windowed(case):
    return ray_check_windowed(case["grid"], case["geom"], case["angles"], case["ranges"], case["rel_pose"],
                              case["pose"], case["params"])


def case_ends(case):
    return beam_ends(case["geom"], case["angles"], case["ranges"], case["rel_pose"], case["pose"], case["params"])


def case_walks(case):
    return beam_walks(case["geom"], case["angles"], case["ranges"], case["rel_pose"], case["pose"], case["params"])


def other_cells(rec):
    return rec["cells"] - rec["cells_free"] - rec["cells_unknown"] - rec["cells_near"] - rec["cells_blocking"]


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


# ---- far frames: up to 2^20 cells between sensor, hit point and map (the bound of include/csm_hip.h) ----

FAR_CELLS = 2 ** 20
FAR_MAX = RES * FAR_CELLS            # the largest usable_range_max the exact geometry takes


def _aimed(S, targets):
    """Angles and ranges of beams from the sensor pose S to the points `targets`."""
    return ([math.atan2(ty - S[1], tx - S[0]) - S[2] for tx, ty in targets],
            [math.hypot(tx - S[0], ty - S[1]) for tx, ty in targets])


def _far(name, grid, angles, ranges, pose, aims, bits, scale, **kw):
    c = _case(name, grid, angles, ranges, pose, aims, subpixel_scale=scale,
              **dict(dict(usable_range_max=FAR_MAX), **kw))
    c["product_bits"] = bits         # the case's largest product is at least 2^bits
    return c


def largest_case_product(case):
    scale = case["params"]["subpixel_scale"]
    return max([largest_product(w, scale) for w in case_ends(case) if w is not None] + [0])


def far_cases():
    cases = []
    g = room(40, 48)
    half = math.pi / 2
    n = FAR_CELLS - 3
    inside = [(30.0, 20.0), (12.3, 25.7), (40.6, 3.2), (7.1, 33.4)]      # cells the beams from outside end in

    def back(tag, sensor_cell, axis_angle, scale, targets, axis_cells, aims):
        S = _at(*sensor_cell) + (0.0,)
        a, r = _aimed(S, [_at(*t) for t in targets])
        # one beam exactly along the axis, ending inside the map
        a.append(axis_angle)
        r.append(axis_cells * RES)
        return _far("far_%s_s%d" % (tag, scale), g, a, r, S, aims, 36 if scale > 1 else 18, scale)

    deep = lambda r: (r["walked"] == r["usable"] == 5 and r["end_inside"] == 5 and r["cells_free"] > 0
                      and r["cells_unknown"] > 0 and r["blocked"] > 0)
    # from the low side a ray of less than 2^20 cells reaches the map's first three columns / rows only
    rim = lambda r: r["walked"] == r["usable"] == 5 and r["end_inside"] == r["end_unknown"] == 5
    near_x, near_y = [(1.0, 20.0), (0.3, 25.7), (2.2, 3.2), (1.6, 33.4)], [(20.0, 1.0), (25.7, 0.3), (3.2, 2.2), (41.4, 1.6)]
    for scale in (512, 1):
        cases.append(back("from_plus_x", (n, 20), math.pi, scale, inside, n - 20, deep))
        cases.append(back("from_minus_x", (-n, 20), 0.0, scale, near_x, n + 1.2, rim))
        cases.append(back("from_minus_x_deep", (60 - n, 20), 0.0, scale, inside, n - 30, deep))
        cases.append(back("from_plus_y", (20, n), -half, scale, inside, n - 20, deep))
        cases.append(back("from_minus_y", (20, -n), half, scale, near_y, n + 1.2, rim))
        cases.append(back("from_minus_y_deep", (20, 60 - n), half, scale, inside, n - 30, deep))
    out_angles = [0.0, half, math.pi, -half, 0.3, 2.0, -2.5, -0.9]
    cx, cy = _at(24, 20)
    for scale in (512, 1, 100):
        cases.append(_far("far_outward_s%d" % scale, g, out_angles, [(FAR_CELLS - 5) * RES] * 8,
                          (cx + 0.013, cy - 0.021, 0.0),
                          lambda r: r["walked"] == 8 and r["blocked"] == 8 and r["end_inside"] == 0
                          and r["cells_free"] > 0 and r["cells_unknown"] > 0,
                          {512: 56, 100: 53, 1: 38}[scale], scale))
    h = FAR_CELLS // 2
    crossings = [("along_x_rising", (-h, 13), (h - 20, 27)), ("along_x_falling", (-h, 27), (h - 20, 13)),
                 ("along_y_rising", (17, -h), (31, h - 20)), ("along_y_falling", (31, -h), (17, h - 20)),
                 ("diagonal_rising", (-700000, -700000), (40048, 40040)),
                 ("diagonal_falling", (-700000, 700040), (40048, -40000))]
    for scale in (512, 1):
        for tag, src, dst in crossings:
            S = _at(*src) + (0.0,)
            a, r = _aimed(S, [_at(*dst)])
            cases.append(_far("far_crossing_%s_s%d" % (tag, scale), g, a, r, S,
                              lambda r: r["walked"] == 1 and r["end_inside"] == 0 and r["cells"] >= 40
                              and r["cells_free"] > 0 and r["blocked"] == 1,
                              {512: 55, 1: 38}[scale] if "diagonal" in tag else {512: 40, 1: 22}[scale], scale))
        cases.append(_far("far_miss_s%d" % scale, g, [math.pi, math.pi + 1e-4, -half], [(FAR_CELLS - 5) * RES] * 3,
                          _at(n, 500) + (0.0,),
                          lambda r: r["usable"] == 3 and r["walked"] == 0 and r["cells"] == 0, 0, scale))
    # a geometry that is not exact, the sensor off the robot
    geom, rel = (0.05, -1.5137, -0.9219), (0.11, -0.07, 0.3)
    pose = (-45000.417, 37.233, -0.4)
    S = api.host_compound(pose, rel)
    a, r = _aimed(S, [_at(c, w, geom) for c, w in inside + [(23.9, 38.6), (46.2, 11.1)]])
    cases.append(_far("far_inexact_offset_sensor", g, a, r, pose,
                      lambda r: r["walked"] == 6 and r["end_inside"] == 6 and r["cells_free"] > 0
                      and r["cells_unknown"] > 0, 40, 100, geom=geom, rel_pose=rel, usable_range_max=0.05 * FAR_CELLS))
    return cases


# ---- clip edges at ordinary distances ----

def speckled(rows, cols, seed):
    """Every class in every neighbourhood: a wrong cell shows in some counter."""
    rng = np.random.RandomState(seed)
    return rng.choice(np.array([0, FREE, FREE, FREE, OTHER, WALL], np.uint16), size=(rows, cols))


def _cells_in(w, shape):
    return [(x, y) for x, y in w["cells"] if 0 <= x < shape[1] and 0 <= y < shape[0]]


def _outside(p, scale, shape):
    """Which side(s) of the map the sub-pixel point p lies beyond: (-1 | 0 | 1, -1 | 0 | 1)."""
    x, y = p[0] // scale, p[1] // scale
    return ((x >= shape[1]) - (x < 0), (y >= shape[0]) - (y < 0))


def _to_cells(sensor_cell, target_cells, theta=0.0, geom=GEOM):
    S = _at(*sensor_cell, geom=geom) + (theta,)
    a, r = _aimed(S, [_at(*t, geom=geom) for t in target_cells])
    return a, r, S


def clip_cases():
    cases = []
    small, big, strip = speckled(17, 23, 31), speckled(70, 65, 32), speckled(3, 129, 33)
    scale = PARAMS["subpixel_scale"]

    def all_from(side, shape):
        return lambda walks: all(w is None or _outside(w["s"], scale, shape) == side for w in walks)

    fan_aims = lambda r: r["usable"] > r["walked"] > 0 and r["cells"] > 0
    # the sensor beyond the high edges of the larger map
    for tag, cell, side in (("high_x", (95, 35), (1, 0)), ("high_y", (30, 95), (0, 1)), ("high_both", (77, 85), (1, 1))):
        a, r = _fan(24, 5 * RES, 90 * RES, seed=40)
        cases.append(_case("clip_sensor_beyond_%s" % tag, big, a, r, _at(*cell) + (0.3,), fan_aims,
                           all_from(side, big.shape), usable_range_max=100.0))
    # fans from the eight outside directions of the small map
    for ix, col in ((-1, -9), (0, 11), (1, 32)):
        for iy, row in ((-1, -7), (0, 8), (1, 24)):
            if ix or iy:
                _, r = _fan(24, 3 * RES, 40 * RES, seed=50 + 3 * ix + iy)
                a = math.atan2(8 - row, 11 - col) - 0.3 + np.linspace(-1.2, 1.2, 24)     # an arc about the map
                cases.append(_case("clip_fan_from_%+d_%+d" % (ix, iy), small, a, r, _at(col, row) + (0.3,), fan_aims,
                                   all_from((ix, iy), small.shape)))

    def crosses(shape):
        return lambda walks: all(w is not None and _outside(w["s"], scale, shape) != (0, 0)
                                 and _outside(w["e"], scale, shape) != (0, 0) and len(_cells_in(w, shape)) > 0
                                 for w in walks)

    # both ends outside, the ray crossing the map
    a, r, S = _to_cells((-20.3, 30.1), [(90.2, 37.4), (88.0, 21.7)])
    cases.append(_case("clip_crossing_flat", big, a, r, S, lambda r: r["walked"] == 2 and r["end_inside"] == 0
                       and r["cells"] > 130, crosses(big.shape), usable_range_max=100.0))
    a, r, S = _to_cells((30.2, -25.4), [(34.1, 100.3), (22.6, 98.0)])
    cases.append(_case("clip_crossing_steep", big, a, r, S, lambda r: r["walked"] == 2 and r["end_inside"] == 0
                       and r["cells"] > 140, crosses(big.shape), usable_range_max=100.0))

    def steep(lo_cut, hi_cut):
        def pred(walks):
            ok = True
            for w in walks:
                ys = [y for _, y in w["cells"]]
                ok = ok and _columns(w) in (2, 3) and len(_cells_in(w, big.shape)) > 64
                ok = ok and (min(ys) < 0) == lo_cut and (max(ys) >= big.shape[0]) == hi_cut
            return ok
        return pred

    # two or three columns, more than 64 rows of them inside: the row range cut below, above, on both sides
    a, r, S = _to_cells((30.4, -40.2), [(31.7, 120.3), (32.3, 118.1)])
    cases.append(_case("clip_steep_cut_both", big, a, r, S, lambda r: r["walked"] == 2 and r["cells"] >= 140,
                       steep(True, True), usable_range_max=100.0))
    a, r, S = _to_cells((30.4, -40.2), [(31.7, 68.3), (28.2, 66.6)])
    cases.append(_case("clip_steep_cut_low", big, a, r, S, lambda r: r["walked"] == 2 and r["end_inside"] == 2,
                       steep(True, False), usable_range_max=100.0))
    a, r, S = _to_cells((30.4, 2.6), [(31.7, 120.3), (28.2, 111.0)])
    cases.append(_case("clip_steep_cut_high", big, a, r, S, lambda r: r["walked"] == 2 and r["end_inside"] == 0,
                       steep(False, True), usable_range_max=100.0))
    # more than 64 outside columns, then all 129 of the strip; from either side
    a, r, S = _to_cells((-80.3, 1.2), [(140.4, 1.7), (150.1, 0.4)])
    cases.append(_case("clip_strip_from_the_left", strip, a, r, S, lambda r: r["walked"] == 2 and r["cells"] >= 258,
                       lambda walks: all(w["s"][0] // scale < -64 and w["e"][0] // scale >= 129 for w in walks),
                       usable_range_max=100.0))
    a, r, S = _to_cells((210.6, 1.3), [(-10.2, 0.6), (-30.5, 2.2)])
    cases.append(_case("clip_strip_from_the_right", strip, a, r, S, lambda r: r["walked"] == 2 and r["cells"] >= 258,
                       lambda walks: all(w["s"][0] // scale > 129 + 64 and w["e"][0] // scale < 0 for w in walks),
                       usable_range_max=100.0))
    # start right of end (the closed form swaps the ends): its first column is then the END's. That column
    # outside (hit beyond the low edge), and the sensor's column outside (sensor beyond the high edge)
    a, r, S = _to_cells((10.3, 8.6), [(-12.2, 5.1), (-7.4, 14.9), (-3.3, -6.0)])
    cases.append(_case("clip_swapped_end_column_outside", small, a, r, S,
                       lambda r: r["walked"] == 3 and r["end_inside"] == 0 and r["cells"] > 20,
                       lambda walks: all(w["s"][0] > w["e"][0] and w["e"][0] < 0 for w in walks)))
    a, r, S = _to_cells((40.3, 8.6), [(12.2, 5.1), (7.4, 14.9), (3.3, 1.0)])
    cases.append(_case("clip_swapped_start_column_outside", small, a, r, S,
                       lambda r: r["walked"] == 3 and r["end_inside"] == 3 and r["cells"] > 20,
                       lambda walks: all(w["s"][0] > w["e"][0] and w["s"][0] // scale >= 23 for w in walks)))
    # exact-corner diagonals (as corners_rising / corners_falling) through the map's four corner cells and
    # through a corner on a border; from inside and from outside
    diag = math.sqrt(2.0) * RES
    q = math.pi / 4
    eps = 0.005 * RES

    def through(corner):
        return lambda walks: (all(w is not None and _diagonal(w) for w in walks)
                              and any(corner in w["cells"] for w in walks)
                              and all(len(_cells_in(w, small.shape)) < len(w["cells"]) for w in walks))

    for tag, cell, up, angles, corner in (
            ("rising_low", (5, 5), 1, [-3 * q, q], (0, 0)), ("rising_high", (17, 11), 1, [q, -3 * q], (22, 16)),
            ("falling_low", (17, 5), -1, [-q, 3 * q], (22, 0)), ("falling_high", (5, 11), -1, [3 * q, -q], (0, 16)),
            ("rising_from_outside", (-6, -6), 1, [q, q], (0, 0)), ("falling_from_outside", (-6, 22), -1, [-q, -q], (0, 16))):
        x, y = _at(*cell)
        lengths = [20 * diag, 9 * diag] if "outside" in tag else [11 * diag, 14 * diag]
        cases.append(_case("clip_corner_diagonal_%s" % tag, small, angles, lengths, (x + eps, y + up * eps, 0.0),
                           lambda r: r["walked"] == 2 and r["cells"] > 0, through(corner)))
    # the end cell on the border row or column, and just beyond it
    a, r, S = _to_cells((11.3, 8.4), [(0.1, 8.2), (-0.9, 8.2), (22.1, 7.7), (23.1, 7.7), (11.8, 0.1), (11.8, -0.9),
                                       (10.6, 16.1), (10.6, 17.1), (0.1, 0.1), (-0.9, -0.8), (22.2, 16.3), (23.1, 17.2)])
    cases.append(_case("clip_end_on_and_beyond_the_border", small, a, r, S,
                       lambda r: r["walked"] == 12 and r["end_inside"] == 6 and r["cells"] > 100))
    return cases


# ---- cell values on the thresholds ----

THRESHOLDS = ((10000, 40000), (1, 65535), (30000, 30001))


def threshold_values(free_max, occupied_min):
    return [0, 1, free_max - 1, free_max, free_max + 1, occupied_min - 1, occupied_min, 65535]


def threshold_cases():
    cases = []
    a, r = _fan(90, 8.0 * RES, 38.0 * RES, seed=5)
    px, py = _at(30, 20)
    rr, cc = np.meshgrid(np.arange(41), np.arange(67), indexing="ij")
    for fm, om in THRESHOLDS:
        grid = np.array(threshold_values(fm, om), np.uint16)[(cc + 3 * rr) % 8]
        for tol in (0, 2):
            cases.append(_case("thresholds_%d_%d_tolerance_%d" % (fm, om, tol), grid, a, r,
                               (px + 0.031, py + 0.017, 0.05),
                               lambda r, tol=tol: r["cells_free"] > 0 and r["cells_unknown"] > 0 and r["blocked"] > 0
                               and (r["cells_near"] > 0 or tol == 0),
                               free_max=fm, occupied_min=om, end_tolerance=tol))
    return cases


# ---- batch bookkeeping ----

BOOKKEEPING_COUNTS = [17, 0, 16, 0, 0, 1, 33, 15, 32, 0]


def bookkeeping_cases():
    """One call's queries over three maps (case["grid_index"]), some of them without a beam."""
    grids = [room(40, 48), speckled(17, 23, 31), threshold_cases()[0]["grid"]]
    sensors = [(24.2, 20.4), (-5.3, 8.1), (30.6, 20.7)]
    cases = []
    for i, n in enumerate(BOOKKEEPING_COUNTS):
        k = i % 3
        a, r = _fan(n, 2 * RES, 30 * RES, seed=60 + i) if n else ([], [])
        c = _case("bookkeeping_%d_beams_%d" % (i, n), grids[k], a, r, _at(*sensors[k]) + (0.1 * i,),
                  lambda r, n=n: r["beams"] == r["usable"] == n and (r["walked"] > 0) == (n > 0))
        c["grid_index"] = k
        cases.append(c)
    return cases


def edge_fan_case(n, axis_only=False, seed=70):
    """A sensor exactly on a cell corner of the exact geometry: the axis-aligned beams of the fan end exactly
    on a cell edge (or within a rounding of it), where no projection is certified. axis_only: every beam."""
    a, r = _fan(n, 2 * RES, 15 * RES, seed=seed)
    if axis_only:
        a = (math.pi / 2) * (np.arange(n) % 4) - math.pi
    return _case("edge_fan_%d%s" % (n, "_axis" if axis_only else ""), room(40, 48), a, r,
                 (GEOM[1] + 24 * RES, GEOM[2] + 20 * RES, 0.0), lambda r: r["usable"] == n and r["walked"] == n)


def late_switch_cases():
    a, r = _fan(33, 2 * RES, 15 * RES, seed=71)
    plain = _case("plain_fan_33", room(40, 48), a, r, _at(24.2, 20.4) + (0.2,), lambda r: r["walked"] == 33)
    return [edge_fan_case(16), plain, edge_fan_case(64), edge_fan_case(40, axis_only=True), plain, edge_fan_case(16)]


# ---- a seeded sweep ----

SWEEP_SEEDS = (0, 1, 2, 3, 4, 5)
SWEEP_ROWS, SWEEP_COLS = (1, 2, 3, 17, 64, 65, 70), (1, 2, 63, 64, 65, 129)
SWEEP_BEAMS = (1, 15, 16, 17, 31, 33, 64, 100)


def sweep_cases(seed):
    """48 queries over 6 random grids under one parameter set; case["grid_index"] names the grid."""
    rng = np.random.RandomState(7000 + seed)
    scale = (1, 2, 3, 37, 100, 512)[seed]
    tol = (0, 1, 2, 5, 2, 1)[seed]
    fm, om = THRESHOLDS[seed % 3]
    values = np.array(threshold_values(fm, om) + [FREE, OTHER, WALL], np.uint16)
    grids = [rng.choice(values, size=(int(rng.choice(SWEEP_ROWS)), int(rng.choice(SWEEP_COLS)))) for _ in range(6)]
    rel = (0.11, -0.07, 0.3)
    cases = []
    for q in range(48):
        k = q % 6
        rows, cols = grids[k].shape
        exact = (q // 3) % 2 == 0
        geom = GEOM if exact else (0.05, -1.5137 - 0.0173 * q, -0.9219 + 0.0311 * q)
        res = geom[0]

        def place(extent):
            side = rng.choice(3, p=[0.5, 0.25, 0.25])
            u = rng.uniform(0.0, 200.0)
            return (rng.uniform(0.0, extent), -u, extent + u)[side]

        sensor = (place(cols), place(rows))
        pose = (geom[1] + sensor[0] * res, geom[2] + sensor[1] * res, float(rng.uniform(-math.pi, math.pi)))
        rel_pose = (0.0, 0.0, 0.0) if exact else rel
        S = api.host_compound(pose, rel_pose)
        n = int(rng.choice(SWEEP_BEAMS))
        angles, ranges = np.zeros(n), np.zeros(n)
        for i in range(n):
            if rng.rand() < 0.7:         # towards the map, ending before, in or beyond it
                tx = geom[1] + rng.uniform(-3.0, cols + 3.0) * res
                ty = geom[2] + rng.uniform(-3.0, rows + 3.0) * res
                angles[i] = math.atan2(ty - S[1], tx - S[0]) - S[2]
                ranges[i] = math.hypot(tx - S[0], ty - S[1]) * rng.uniform(0.3, 1.6)
            else:
                angles[i] = rng.uniform(-math.pi, math.pi)
                ranges[i] = rng.uniform(0.5, 120.0) * res
            ranges[i] = min(max(ranges[i], 0.5 * res), 120.0 * res)
            if rng.rand() < 0.03:
                ranges[i] = (float("nan"), 40.0, 0.0)[rng.randint(3)]
        c = _case("sweep_%d_query_%d" % (seed, q), grids[k], angles, ranges, pose, None, geom=geom, rel_pose=rel_pose,
                  subpixel_scale=scale, end_tolerance=tol, free_max=fm, occupied_min=om, usable_range_max=31.0)
        c["grid_index"] = k
        cases.append(c)
    return cases
