"""numpy statement of the likelihood-field definition (include/csm_hip.h), written
independently of the C loop: one shifted copy of the obstacle values per tap of the disc, a running
maximum over the taps. The table comes from math.exp. Shared by the CPU and GPU likelihood tests."""
import functools
import math

import numpy as np

MAX_RADIUS = 16


def radius(sigma, res):
    return int(min(float(MAX_RADIUS), max(1.0, math.ceil(min(3.0 * (sigma / res), 1e9)))))


def kernel(sigma, res, R):
    """T[0 .. R^2]: floor(32768 exp(-d2 res^2 / (2 sigma^2)) + 0.5)."""
    return np.array([int(math.floor(32768.0 * math.exp(-(d2 * (res * res)) / (2.0 * (sigma * sigma))) + 0.5))
                     for d2 in range(R * R + 1)], np.uint32)


def likelihood_map(grid, table, R, occupied_min=32768, keep_unknown=False):
    """out(c) = max(G[c], max over obstacles o within R of 1 + (((G[o] - 1) T[d2]) >> 15)); an unknown cell
    stays 0 under keep_unknown."""
    g = np.asarray(grid, np.uint16).astype(np.int64)
    rows, cols = g.shape
    obst = np.where(g >= occupied_min, g, 0)
    pad = np.zeros((rows + 2 * R, cols + 2 * R), np.int64)
    pad[R:R + rows, R:R + cols] = obst
    spread = np.zeros_like(g)
    for dr in range(-R, R + 1):
        for dc in range(-R, R + 1):
            d2 = dr * dr + dc * dc
            if d2 > R * R:
                continue
            v = pad[R + dr:R + dr + rows, R + dc:R + dc + cols]        # the value of the obstacle at c + (dr, dc)
            s = np.where(v > 0, 1 + (((v - 1) * int(table[d2])) >> 15), 0)
            np.maximum(spread, s, out=spread)
    out = np.maximum(g, spread)
    if keep_unknown:
        out[g == 0] = 0
    assert out.max(initial=0) <= 65535
    return out.astype(np.uint16)


def far_from_obstacles(grid, R, occupied_min=32768):
    """Mask of the cells with no obstacle within R (Euclidean, in cells), by brute force over the obstacles."""
    g = np.asarray(grid)
    rr, cc = np.nonzero(g >= occupied_min)
    far = np.ones(g.shape, bool)
    for r, c in zip(rr, cc):
        r0, r1 = max(0, r - R), min(g.shape[0], r + R + 1)
        c0, c1 = max(0, c - R), min(g.shape[1], c + R + 1)
        y, x = np.ogrid[r0:r1, c0:c1]
        far[r0:r1, c0:c1] &= (y - r) ** 2 + (x - c) ** 2 > R * R
    return far


# ---- the cases both test files run: name -> (grid, R, sigma, res, occupied_min) ----

def _random(shape, seed, density=0.03):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 32768, shape).astype(np.uint16)
    g[rng.random(shape) < 0.4] = 0                                       # unknown cells
    hit = rng.random(shape) < density
    g[hit] = rng.integers(32768, 65535, shape).astype(np.uint16)[hit]    # obstacles, <= 65534
    return g


def _corners(shape, value=50000):
    g = np.zeros(shape, np.uint16)
    g[5:-5, 5:-5] = 9000
    for r in (0, shape[0] - 1):
        for c in (0, shape[1] - 1):
            g[r, c] = value
    return g


def _seams(shape=(97, 131)):
    """Obstacles at rows and columns 31, 32, 33, 63, 64, 65 (tile and halo seams) and on the last row and
    column; every third of them in unknown surroundings."""
    g = np.full(shape, 700, np.uint16)
    g[:, 100:] = 0
    g[70:, :] = 0
    marks = (31, 32, 33, 63, 64, 65)
    for i, r in enumerate(marks):
        for k, c in enumerate(marks):
            if (i + k) % 2 == 0:
                g[r, c] = 33000 + 1000 * i + 100 * k
    g[shape[0] - 1, 7] = 40000
    g[shape[0] - 1, shape[1] - 1] = 65534
    g[12, shape[1] - 1] = 45000
    g[0, 64] = 36000
    return g


@functools.lru_cache(maxsize=None)
def grid_of(name):
    from csm_hip import synth
    if name == "random16":
        return _random((16, 16), 1, 0.05)
    if name == "random37x53":
        return _random((37, 53), 2)
    if name == "random65x130":
        return _random((65, 130), 3)
    if name == "all_unknown":
        return np.zeros((20, 33), np.uint16)
    if name == "all_obstacle":
        return _random((20, 33), 4, 0.0) // 2 + np.uint16(40000)
    if name == "corners":
        return _corners((41, 70))
    if name == "threshold":
        g = np.full((24, 40), 100, np.uint16)
        g[4, 4] = 32768             # exactly occupied_min: an obstacle
        g[4, 30] = 32767            # occupied_min - 1: not one
        g[18, 20] = 0
        g[19, 5] = 32768
        g[19, 6] = 0
        return g
    if name == "extremes":
        g = np.zeros((30, 30), np.uint16)
        g[10:20, 10:20] = 1         # the smallest known value, around ...
        g[15, 15] = 65534           # ... the largest obstacle
        g[3, 3] = 1
        return g
    if name == "seams":
        return _seams()
    if name == "dense64":
        return _random((64, 64), 5, 0.6)
    if name == "csm_case0":
        return synth.csm_case(0)["grid"]
    if name in _EDGE_GRIDS:
        return _EDGE_GRIDS[name]()
    raise KeyError(name)


# (grid name, R): sigma = R / 3 cells at res 0.05 unless given
CPU_CASES = [("random16", 1), ("random16", 3), ("random37x53", 1), ("random37x53", 3), ("random37x53", 16),
             ("random65x130", 3), ("random65x130", 16), ("all_unknown", 3), ("all_obstacle", 3), ("corners", 1),
             ("corners", 16), ("threshold", 3), ("extremes", 3), ("extremes", 16), ("csm_case0", 3)]
GPU_EXTRA_CASES = [("seams", 1), ("seams", 3), ("seams", 16), ("dense64", 16), ("dense64", 3)]
RES = 0.05


def sigma_of(R):
    return R * RES / 3.0


def occupied_min_of(name):
    return 1 if name == "extremes" else 32768      # "extremes": the value-1 cells are obstacles too


@functools.lru_cache(maxsize=None)
def expected(name, R, keep_unknown):
    """(grid, table, reference output) of a case; computed once per session."""
    g = grid_of(name)
    t = kernel(sigma_of(R), RES, R)
    out = likelihood_map(g, t, R, occupied_min_of(name), keep_unknown)
    for a in (g, t, out):
        a.setflags(write=False)
    return g, t, out


# ---- edge cases: the numbers the kernel's index arithmetic branches on ----

TILE_ROWS, TILE_COLS = 32, 64          # one workgroup's output tile


def first_known(grid):
    """(smallest row, smallest column) holding a non-zero cell; (rows, cols) if there is none."""
    g = np.asarray(grid)
    rr, cc = np.nonzero(g)
    return (int(rr.min()), int(cc.min())) if rr.size else (int(g.shape[0]), int(g.shape[1]))


def halo_counts(grid, R, occupied_min=32768):
    """[row tiles, column tiles]: the obstacles in rows [32 i - R, 32 i + 32 + R) by columns [64 j - R,
    64 j + 64 + R), clipped to the map: the number a workgroup compares with (2R + 1)^2 to choose between
    walking its obstacle list and visiting the taps of the disc."""
    obst = np.asarray(grid).astype(np.int64) >= occupied_min
    rows, cols = obst.shape
    nr, nc = -(-rows // TILE_ROWS), -(-cols // TILE_COLS)
    out = np.zeros((nr, nc), np.int64)
    for i in range(nr):
        for j in range(nc):
            out[i, j] = obst[max(0, TILE_ROWS * i - R):TILE_ROWS * (i + 1) + R,
                             max(0, TILE_COLS * j - R):TILE_COLS * (j + 1) + R].sum()
    return out


def switch_count(R):
    return (2 * R + 1) ** 2


def disc_cells(R):
    """The number of integer points with dr^2 + dc^2 <= R^2: 1 + 4 sum_{x = 0 .. R} floor(sqrt(R^2 - x^2))
    (the centre, then one quadrant's points with dr >= 0, dc > 0, turned four times)."""
    return 1 + 4 * sum(math.isqrt(R * R - x * x) for x in range(R + 1))


def table_of(kind, R):
    """"gauss": kernel(sigma_of(R)); "flat": 32768 throughout, the output is the disc; "zero": 0 throughout,
    every cell of a disc becomes 1 at least; "ramp": 32768 - 97 d2 mod 32768, a different value at every d2."""
    if kind == "gauss":
        return kernel(sigma_of(R), RES, R)
    if kind == "flat":
        return np.full(R * R + 1, 32768, np.uint32)
    if kind == "zero":
        return np.zeros(R * R + 1, np.uint32)
    if kind == "ramp":
        return np.array([32768 - (97 * d2) % 32768 for d2 in range(R * R + 1)], np.uint32)
    raise KeyError(kind)


SINGLE_AT = (20, 37)


def _single(value):
    g = np.zeros((48, 80), np.uint16)
    g[SINGLE_AT] = value
    return g


def _line(n, marks):
    """n cells, known (700) and unknown in runs of four and three, obstacles at the marks."""
    g = np.where(np.arange(n) % 7 < 4, 700, 0).astype(np.uint16)
    for k, i in enumerate(marks):
        g[i] = 40000 + 1000 * k
    return g


def _scatter(g, cells, seed):
    """Obstacles (random in 32768..65534) on the listed flat indices of g."""
    rng = np.random.default_rng(seed)
    g.reshape(-1)[cells] = rng.integers(32768, 65535, len(cells)).astype(np.uint16)
    return g


def _switch(R, extra):
    shape = (TILE_ROWS, TILE_COLS)                       # one tile: its halo lies outside the map
    cells = np.random.default_rng(100 + R).permutation(shape[0] * shape[1])[:switch_count(R) + extra]
    return _scatter(_random(shape, 110 + R, 0.0), cells, 120 + R)


LAST_ROWS = (18, 21, 24, 27, 30)


def _switch_16_last():
    """(2 x 16 + 1)^2 + 1 obstacles of which the last the kernel meets cannot go missing unseen. The tile is
    staged row by row, and the list stores 1089 entries: a walk of the list at this count loses one of the
    obstacles met last. Rows 18 .. 31 hold 110 obstacles of 65534 on a lattice (rows 18, 21, .., 30, every
    third column) among known cells of 700: the cell under each of them has no other obstacle within two
    cells, so it takes its value from that obstacle alone. Rows 0 .. 15 hold the other 980."""
    g = np.full((TILE_ROWS, TILE_COLS), 700, np.uint16)
    g[:16] = _random((16, TILE_COLS), 140, 0.0)
    _scatter(g, np.random.default_rng(141).permutation(16 * TILE_COLS)[:switch_count(16) + 1 - 110], 142)
    for r in LAST_ROWS:
        g[r, ::3] = 65534
    return g


RIM_AT = (10, 5)


def _dense_rim():
    """64 x 64: columns 40 .. 63 of rows 0 .. 47 are all obstacles (1152, more than (2 x 16 + 1)^2, all in the
    halo of the upper tile at every radius: the taps path), and one obstacle stands alone at RIM_AT, at least
    19 columns from the block: the cells around it show the disc the taps path draws, rim included."""
    g = _random((64, 64), 150, 0.0)
    g[:48, 40:] = np.random.default_rng(151).integers(32768, 65535, (48, 24)).astype(np.uint16)
    g[RIM_AT] = 50000
    return g


def _switch_two_tiles(R=3):
    """32 x 128: the left tile sees columns 0 .. 63 + R, the right one 64 - R .. 127. 45 obstacles only the
    left tile sees, 5 both see, 44 only the right one: (2R + 1)^2 + 1 = 50 on the left, 49 on the right."""
    shape = (TILE_ROWS, 2 * TILE_COLS)
    rng = np.random.default_rng(130)
    c = np.arange(shape[0] * shape[1]) % shape[1]                 # the column of every flat index
    pick = lambda mask, n: rng.permutation(np.flatnonzero(mask))[:n]
    cells = np.concatenate([pick(c < TILE_COLS - R, 45), pick((c >= TILE_COLS - R) & (c < TILE_COLS + R), 5),
                            pick(c >= TILE_COLS + R, 44)])
    return _scatter(_random(shape, 131, 0.0), cells, 132)


LOW_KNOWN_OBSTACLE = (10, 12)


def _low_known():
    """random65x130 without its first 9 rows and 11 columns, one obstacle 1 row and 1 column inside what is
    left: with keep_unknown = 0 its disc (R = 3) reaches into the emptied band."""
    g = _random((65, 130), 3).copy()
    g[:9, :] = 0
    g[:, :11] = 0
    g[LOW_KNOWN_OBSTACLE] = 52000
    return g


def _room200():
    from csm_hip import synth
    return synth.csm_case(1, rows=200, cols=200)["grid"]


_EDGE_GRIDS = {
    "single": lambda: _single(50000),
    "single_65535": lambda: _single(65535),
    "line1xN": lambda: _line(200, (0, 199, 63, 64, 65)).reshape(1, 200),
    "lineNx1": lambda: _line(200, (0, 199, 63, 64, 65, 31, 32, 33)).reshape(200, 1),
    "one_cell": lambda: np.full((1, 1), 50000, np.uint16),
    "switch_1": lambda: _switch(1, 0), "switch_1_plus": lambda: _switch(1, 1),
    "switch_3": lambda: _switch(3, 0), "switch_3_plus": lambda: _switch(3, 1),
    "switch_16": lambda: _switch(16, 0), "switch_16_plus": lambda: _switch(16, 1),
    "switch_two_tiles": _switch_two_tiles,
    "switch_16_last": _switch_16_last,
    "dense_rim": _dense_rim,
    "dense40x70": lambda: _random((40, 70), 6, 0.6),
    "dense60x100": lambda: _random((60, 100), 7, 0.6),
    "room200": _room200,
    "low_known": _low_known,
}

# (grid name, R, table kind, occupied_min)
EDGE_CASES = (
    [("single", R, kind, 32768) for R in (2, 5, 10, 13, 15, 16) for kind in ("flat", "ramp")]
    + [("single", 5, "zero", 32768), ("random37x53", 3, "zero", 32768)]
    + [("single_65535", 3, "flat", 32768), ("single_65535", 3, "gauss", 32768)]
    + [(name, R, "ramp", 32768) for name in ("line1xN", "lineNx1", "one_cell") for R in (1, 16)]
    + [("random37x53", 3, "gauss", 40000), ("random37x53", 3, "gauss", 65535), ("random37x53", 3, "gauss", 70000)]
    + [("switch_%d%s" % (R, plus), R, "ramp", 32768) for R in (1, 3, 16) for plus in ("", "_plus")]
    + [("switch_16_last", 16, "ramp", 32768), ("switch_two_tiles", 3, "ramp", 32768)]
    + [("dense40x70", 3, "ramp", 32768), ("dense40x70", 16, "ramp", 32768), ("dense60x100", 16, "ramp", 32768)]
    + [("dense_rim", R, "flat", 32768) for R in (5, 10, 13, 15, 16)] + [("dense_rim", 16, "ramp", 32768)]
    + [("room200", 16, "gauss", 32768)]
    + [("low_known", 3, "gauss", 32768)])
# the earlier tables in the same form
ALL_CASES = [(name, R, "gauss", occupied_min_of(name)) for name, R in CPU_CASES + GPU_EXTRA_CASES] + EDGE_CASES


@functools.lru_cache(maxsize=None)
def edge_expected(name, R, kind, occupied_min, keep_unknown):
    """(grid, table, reference output) of an EDGE_CASES / ALL_CASES entry; computed once per session."""
    g = grid_of(name)
    t = table_of(kind, R)
    out = likelihood_map(g, t, R, occupied_min, keep_unknown)
    for a in (g, t, out):
        a.setflags(write=False)
    return g, t, out
