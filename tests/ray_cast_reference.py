"""Virtual scans (include/csm_hip.h, csm_ray_cast) in numpy / Python integers: the contract every other layer
equals. The cells of a beam come from ray_check_reference.beam_walks (oracle.ray_cells, the step-by-step
BresenhamScaled, after the whole-cell move), are read from the sensor's end, and the first stopping cell is
the record. Also the named cases of tests/test_cpu_ray_cast.py and tests/test_gpu_ray_cast.py: hand-made grids
of at most 200 rows x 160 columns, at most 16 beams each, each with what it aims at. Every directional case
exists twice: as written (the sensor at the low-x end of its rays) and mirrored in x (the sensor at the high-x
end, where the reference swaps its end points and the device enumerates columns downwards)."""
import math

import numpy as np

import ray_check_reference as R
from csm_hip import api

WALL, FREE = R.WALL, R.FREE
RES, GEOM = R.RES, R.GEOM
NONE, OCCUPIED, UNKNOWN = api.CAST_NONE, api.CAST_OCCUPIED, api.CAST_UNKNOWN
PARAMS = dict(range_max=60.0, range_min=0.0, subpixel_scale=100, occupied_min=40000, unknown_stops=0)
ZERO = (0.0, 0.0, 0.0)
HALF = math.pi / 2


def params(**kw):
    p = dict(PARAMS)
    p.update(kw)
    return p


def limits(n, ranges, range_max):
    """Per beam None (not cast) or its limit."""
    if ranges is None:
        return [range_max] * n
    return [(r if r < range_max else range_max) if r > 0 else None
            for r in np.asarray(ranges, np.float64).tolist()]


def min_dist2(range_min, res, scale):
    m = math.ceil(2.0 * range_min / (res / scale)) if math.isfinite(range_min) else 2 ** 31
    return min(int(m), 2 ** 31) ** 2


def dist2(cell, s, scale):
    dx = 2 * cell[0] * scale + scale - 2 * s[0] - 1
    dy = 2 * cell[1] * scale + scale - 2 * s[1] - 1
    return dx * dx + dy * dy


def pose_walks(geom, angles, ranges, pose, prm):
    """Per beam None (not cast) or dict(s, e, cells): W in the order of the cast, from the sensor's cell."""
    lim = limits(len(angles), ranges, prm["range_max"])
    assert tuple(api.host_compound(pose, ZERO)) == tuple(float(v) for v in pose)
    cast = [i for i, v in enumerate(lim) if v is not None]
    walks = R.beam_walks(geom, [angles[i] for i in cast], [lim[i] for i in cast], ZERO, pose,
                         dict(usable_range_min=0.0, usable_range_max=math.inf, subpixel_scale=prm["subpixel_scale"]))
    out = [None] * len(lim)
    scale = prm["subpixel_scale"]
    for i, w in zip(cast, walks):
        sensor = (w["s"][0] // scale, w["s"][1] // scale)
        cells = list(w["cells"])
        w["sensor_is_an_end"] = sensor in (cells[0], cells[-1])
        w["reversed"] = cells[0] != sensor
        if w["reversed"]:
            cells.reverse()
        w["cells"] = cells
        out[i] = w
    return out


def cast(grid, geom, angles, ranges, poses, prm, with_walks=False):
    """CAST_RECORD array (n_poses, n_beams); with_walks also the walks of every pose."""
    g = np.asarray(grid)
    rows, cols = g.shape
    scale = prm["subpixel_scale"]
    m2 = min_dist2(prm["range_min"], geom[0], scale)
    poses = np.asarray(poses, np.float64).reshape(-1, 3)
    out = np.zeros((poses.shape[0], len(angles)), api.CAST_RECORD)
    all_walks = []
    for p, pose in enumerate(poses.tolist()):
        walks = pose_walks(geom, list(np.asarray(angles, np.float64).tolist()), ranges, tuple(pose), prm)
        all_walks.append(walks)
        for i, w in enumerate(walks):
            if w is None:
                continue
            for (x, y) in w["cells"]:
                if not (0 <= x < cols and 0 <= y < rows):
                    continue
                d2 = dist2((x, y), w["s"], scale)
                if d2 < m2:
                    continue
                v = int(g[y, x])
                kind = OCCUPIED if v >= prm["occupied_min"] else UNKNOWN if (prm["unknown_stops"] and v == 0) else NONE
                if kind != NONE:
                    out[p, i] = (x, y, v, kind, d2)
                    break
    return (out, all_walks) if with_walks else out


def cast_case(case, with_walks=False):
    return cast(case["grid"], case["geom"], case["angles"], case["ranges"], case["poses"], case["params"], with_walks)


def stop_index(w, rec):
    """The place of the record's cell in the walk (from the sensor), among the cells inside the map only."""
    return None if rec["kind"] == NONE else w["cells"].index((int(rec["cell_x"]), int(rec["cell_y"])))


# ---- named cases ----

def _at(col, row, fx=0.5, fy=0.5, geom=GEOM):
    """The map-local position of the point (fx, fy) of cell (col, row); (0.5, 0.5) is its centre."""
    return (geom[1] + (col + fx) * geom[0], geom[2] + (row + fy) * geom[0])


def _case(name, grid, angles, poses, aims, ranges=None, geom=GEOM, **prm):
    return dict(name=name, grid=np.ascontiguousarray(grid, np.uint16), geom=geom,
                angles=np.asarray(angles, np.float64), ranges=None if ranges is None else np.asarray(ranges, np.float64),
                poses=np.asarray(poses, np.float64).reshape(-1, 3), params=params(**prm), aims=aims)


def _mirrored(c):
    """The same scene seen in a mirror x -> -x: every ray's sensor is now at its other end in x."""
    cols = c["grid"].shape[1]
    res, off_x, _ = c["geom"]
    poses = c["poses"].copy()
    poses[:, 0] = (2 * off_x + cols * res) - poses[:, 0]
    poses[:, 2] = math.pi - poses[:, 2]
    m = dict(c, name=c["name"] + "_mirrored", grid=np.ascontiguousarray(c["grid"][:, ::-1]), poses=poses,
             angles=-c["angles"], mirrored=True)
    return m


def _free(rows, cols):
    return np.full((rows, cols), FREE, np.uint16)


def _cells(recs):
    return [(int(r["cell_x"]), int(r["cell_y"])) if r["kind"] != NONE else None for r in recs.reshape(-1)]


def _kinds(recs):
    return [int(k) for k in recs["kind"].reshape(-1)]


def _x(case, col):
    """Column `col` of the case as written, in the case's own grid."""
    return case["grid"].shape[1] - 1 - col if case.get("mirrored") else col


def named_cases():
    """Each aims(case, records, walks) -> bool says what the case is there for, in terms of the reference."""
    out = []

    def both(c):
        out.append(c)
        out.append(_mirrored(c))

    # --- directions ---
    g = _free(40, 100)
    g[:, 70] = WALL
    both(_case("horizontal", g, [0.0, math.pi], [_at(10, 20) + (0.0,)],
               lambda c, r, w: _cells(r) == [(_x(c, 70), 20), None] and len({y for _, y in w[0][0]["cells"]}) == 1))
    g = _free(200, 30)
    g[150, :] = WALL
    both(_case("vertical_more_than_64_rows", g, [HALF, -HALF, -HALF], [_at(15, 20) + (0.0,), _at(15, 180) + (0.0,)],
               lambda c, r, w: _cells(r) == [(_x(c, 15), 150), None, None, None, (_x(c, 15), 150), (_x(c, 15), 150)]
               and stop_index(w[0][0], r[0, 0]) == 130 and len({x for x, _ in w[0][0]["cells"]}) == 1))
    g = _free(100, 100)
    g[:10, :] = g[90:, :] = WALL
    g[:, :10] = g[:, 90:] = WALL
    diag = lambda w: all(a[0] != b[0] and a[1] != b[1] for a, b in zip(w["cells"], w["cells"][1:]))
    both(_case("corners_rising", g, [math.pi / 4, -3 * math.pi / 4], [_at(20, 20, 0.505, 0.505) + (0.0,)],
               lambda c, r, w: _cells(r) == [(_x(c, 90), 90), (_x(c, 9), 9)] and all(diag(v) for v in w[0])))
    both(_case("corners_falling", g, [-math.pi / 4, 3 * math.pi / 4], [_at(20, 80, 0.505, 0.495) + (0.0,)],
               lambda c, r, w: _cells(r) == [(_x(c, 90), 10), (_x(c, 10), 90)] and all(diag(v) for v in w[0])))

    # --- two walls on one ray: the nearer one wins ---
    g = _free(30, 160)
    g[:, 60] = g[:, 100] = WALL
    both(_case("two_walls_in_two_rounds", g, [0.01, -0.013], [_at(5, 15) + (0.0,)],
               lambda c, r, w: [x for x, _ in _cells(r)] == [_x(c, 60)] * 2
               and stop_index(w[0][0], r[0, 0]) < 64 <= w[0][0]["cells"].index((_x(c, 100), 15 + 1))))
    g = _free(30, 160)
    g[:, 15] = g[:, 55] = WALL
    both(_case("two_walls_either_side_of_lane_32", g, [0.01, -0.013], [_at(5, 15) + (0.0,)],
               lambda c, r, w: [x for x, _ in _cells(r)] == [_x(c, 15)] * 2
               and stop_index(w[0][0], r[0, 0]) < 32 < w[0][0]["cells"].index((_x(c, 55), 15)) < 64))

    # --- long rays: the exit must not fire early ---
    g = _free(30, 160)
    g[:, 150] = WALL
    both(_case("wall_in_the_third_round", g, [0.005, -0.004], [_at(3, 15) + (0.0,)],
               lambda c, r, w: [x for x, _ in _cells(r)] == [_x(c, 150)] * 2 and stop_index(w[0][0], r[0, 0]) >= 128))
    both(_case("no_wall_in_three_rounds", _free(30, 160), [0.005, -0.004], [_at(3, 15) + (0.0,)],
               lambda c, r, w: _kinds(r) == [NONE, NONE] and len({x for x, _ in w[0][0]["cells"]}) > 128))

    # --- steep rays: few columns, several ballots per round ---
    g = _free(200, 31)
    g[100, :] = WALL
    steep = math.atan2(70.0, 0.6)
    both(_case("steep_hit_in_the_second_group", g, [steep, steep + 0.004], [_at(15, 5) + (0.0,)],
               lambda c, r, w: [y for _, y in _cells(r)] == [100, 100] and 64 <= stop_index(w[0][0], r[0, 0]) < 128
               and 2 <= len({x for x, _ in w[0][0]["cells"]}) <= 3 and len(w[0][0]["cells"]) > 128))
    both(_case("steep_downwards", g, [-steep, -steep - 0.004], [_at(15, 195) + (0.0,)],
               lambda c, r, w: [y for _, y in _cells(r)] == [100, 100] and 64 <= stop_index(w[0][0], r[0, 0]) < 128))

    # --- the end cell and beyond ---
    g = _free(40, 100)
    g[:, 40] = WALL
    both(_case("end_cell_and_limits", g, [0.0] * 7, [_at(10, 20) + (0.0,)],
               lambda c, r, w: _cells(r) == [(_x(c, 40), 20), None, (_x(c, 40), 20), (_x(c, 40), 20), None, None, None]
               and w[0][0]["cells"][-1] == (_x(c, 40), 20) and w[0][1]["cells"][-1] == (_x(c, 39), 20)
               and w[0][4] is None and w[0][5] is None and w[0][6] is None,
               # a wall exactly on E; one cell beyond E; a limit longer than range_max; one shorter but past the
               # wall; zero, negative, NaN
               ranges=[30 * RES, 29 * RES, 1000.0, 45 * RES, 0.0, -1.0, float("nan")], range_max=50 * RES))

    # --- where the sensor is ---
    g = _free(40, 100)
    g[:, 10] = g[:, 30] = WALL
    # the sensor on the centre of a sub-pixel, as its mirror image is: the distances are the same both ways
    near = 3999 * (RES / 100) / 2          # centre of the sensor's sub-pixel to the centre of cell 30
    both(_case("sensor_in_a_wall", g, [0.0], [_at(10, 20, 0.505) + (0.0,)],
               lambda c, r, w: _cells(r) == [(_x(c, 10), 20)] and int(r[0, 0]["dist2"]) == 2))
    both(_case("range_min_below_the_next_wall", g, [0.0], [_at(10, 20, 0.505) + (0.0,)],
               lambda c, r, w: _cells(r) == [(_x(c, 30), 20)] and int(r[0, 0]["dist2"]) == 3999 ** 2 + 1,
               range_min=near - 1e-6))
    both(_case("range_min_above_the_next_wall", g, [0.0], [_at(10, 20, 0.505) + (0.0,)],
               lambda c, r, w: _kinds(r) == [NONE], range_min=near + 1e-3))
    room = R.room(80, 96)
    fan = -math.pi + 2 * math.pi * np.arange(16) / 16 + 0.01
    both(_case("sensor_outside_low", room, fan, [_at(-9, -7) + (0.3,)],
               lambda c, r, w: OCCUPIED in _kinds(r) and NONE in _kinds(r) and w[0][0]["s"][1] < 0))
    both(_case("sensor_outside_high", room, fan, [_at(104, 85) + (0.3,)],
               lambda c, r, w: OCCUPIED in _kinds(r) and NONE in _kinds(r) and w[0][0]["s"][1] > 80 * 100))
    both(_case("rays_that_leave_the_map", _free(40, 60), fan, [_at(30, 20) + (0.0,)],
               lambda c, r, w: set(_kinds(r)) == {NONE}))

    # --- unknown cells ---
    g = _free(40, 100)
    g[:, 30:33] = 0
    g[:, 50] = WALL
    for stops in (0, 1):
        both(_case("unknown_before_a_wall_stops_%d" % stops, g, [0.0, 0.02], [_at(10, 20) + (0.0,)],
                   lambda c, r, w, stops=stops: [x for x, _ in _cells(r)] == [_x(c, 30 if stops else 50)] * 2
                   and _kinds(r) == [UNKNOWN if stops else OCCUPIED] * 2, unknown_stops=stops))
    both(_case("unknown_only_outside_the_map", _free(40, 60), fan, [_at(30, 20) + (0.0,), _at(-5, 20) + (0.0,)],
               lambda c, r, w: set(_kinds(r)) == {NONE}, unknown_stops=1))

    # --- thresholds ---
    g = _free(40, 100)
    g[:, 40] = 59999
    g[:, 50] = 60000
    g[:, 60] = 65535
    g[:, 20:23] = 0
    both(_case("occupied_min_1", g, [0.0], [_at(21, 20) + (0.0,)],
               lambda c, r, w: _cells(r) == [(_x(c, 23), 20)] and int(r[0, 0]["value"]) == FREE, occupied_min=1))
    both(_case("occupied_min_at_the_value", g, [0.0], [_at(21, 20) + (0.0,)],
               lambda c, r, w: _cells(r) == [(_x(c, 50), 20)], occupied_min=60000))
    both(_case("occupied_min_65535", g, [0.0], [_at(21, 20) + (0.0,)],
               lambda c, r, w: _cells(r) == [(_x(c, 60), 20)] and int(r[0, 0]["value"]) == 65535, occupied_min=65535))

    # --- sub-pixel scales, several poses ---
    odd = R.room(41, 67)
    for scale in (1, 2, 7, 100):
        both(_case("scale_%d" % scale, odd, fan, [_at(30, 20, 0.62, 0.57) + (0.05,), _at(12, 30, 0.1, 0.9) + (2.0,)],
                   lambda c, r, w: set(_kinds(r)) == {OCCUPIED}, subpixel_scale=scale))

    # --- ends exactly on cell edges: the device cannot certify them ---
    g = _free(40, 100)
    g[:, 70] = WALL
    both(_case("ends_on_cell_edges", g, [0.0, HALF, math.pi, -HALF], [_at(10, 20, 0.0, 0.0) + (0.0,)],
               lambda c, r, w: _kinds(r)[0] == OCCUPIED, ranges=[75 * RES, 10 * RES, 2 * RES, 12 * RES]))
    return out


def ends_on_edges(case):
    """How many cast beams of the case have an end point exactly on a sub-pixel edge, on either axis, in the
    reference's own double expressions."""
    res, off_x, off_y = case["geom"]
    scaled = res / case["params"]["subpixel_scale"]
    n = 0
    for pose in case["poses"].tolist():
        lim = limits(len(case["angles"]), case["ranges"], case["params"]["range_max"])
        for a, r in zip(case["angles"].tolist(), lim):
            if r is None:
                continue
            qx = (pose[0] + r * math.cos(pose[2] + a) - off_x) / scaled
            qy = (pose[1] + r * math.sin(pose[2] + a) - off_y) / scaled
            n += qx == math.floor(qx) or qy == math.floor(qy)
    return n


# ---- seeded fuzz: speckled grids, sensors inside and outside, every rule at once ----

def fuzz_cases(n_cases=6, n_poses=40, n_beams=16, seed=7):
    out = []
    for k in range(n_cases):
        rng = np.random.RandomState(seed + k)
        rows, cols = int(rng.randint(20, 90)), int(rng.randint(20, 90))
        g = np.full((rows, cols), FREE, np.uint16)
        speck = rng.rand(rows, cols)
        g[speck < 0.03] = WALL
        g[speck > 0.95] = 0
        geom = (0.05, -1.5137, -0.9219) if k % 2 else GEOM
        res = geom[0]
        poses = np.stack([geom[1] + res * rng.uniform(-15, cols + 15, n_poses),
                          geom[2] + res * rng.uniform(-15, rows + 15, n_poses),
                          rng.uniform(-math.pi, math.pi, n_poses)], axis=1)
        angles = rng.uniform(-math.pi, math.pi, n_beams)
        ranges = None if k % 3 == 0 else rng.uniform(-0.2, 60, n_beams) * res
        out.append(_case("fuzz_%d" % k, g, angles, poses, None, ranges=ranges, geom=geom, range_max=50 * res,
                         range_min=(0.0, 1.3 * res, 4.0 * res)[k % 3], subpixel_scale=(100, 7, 1, 2, 100, 512)[k % 6],
                         unknown_stops=k % 2))
    return out
