"""numpy statement of the distance-field definition (include/csm_hip.h): brute force over the
obstacles in ascending index order with a strict `<`, so that the smallest index wins a tie. Independent of
the two-pass form the library uses. The table comes from math.exp. Shared by the CPU and GPU distance tests;
the cases are small because the brute force is cells x obstacles."""
import functools
import math

import numpy as np

MAX_RADIUS = 255
NONE = 0xFFFFFFFF
RES = 0.05
RUN_ROWS = 4            # rows of one workgroup of the row pass (kDtRun)
WIDE_COLS = 8192        # the widest map with one wavefront per staged row (kDtWide)
MAX_SIDE = 32767        # the most rows and the most columns a map may have
LDS_HEAD = 16           # bytes ahead of the staged rows (kDtHead)


def staged_bytes(cols):
    """Dynamic LDS of the row pass for a launch whose widest map has `cols` columns: the head, then four rows
    (one when cols > WIDE_COLS) of int16 slots, the row rounded up to 8 slots."""
    return LDS_HEAD + (4 if cols <= WIDE_COLS else 1) * ((cols + 7) & ~7) * 2


def kernel(sigma, res, R, peak=65534, floor_value=1):
    """T[0 .. R^2]: floor_value + floor((peak - floor_value) exp(-d2 res^2 / (2 sigma^2)) + 0.5)."""
    return np.array([floor_value + int(math.floor((peak - floor_value) *
                                                  math.exp(-(d2 * (res * res)) / (2.0 * (sigma * sigma))) + 0.5))
                     for d2 in range(R * R + 1)], np.uint16)


def radius(sigma, res):
    return int(min(float(MAX_RADIUS), max(1.0, math.ceil(3.0 * (sigma / res)))))


def transform(grid, occupied_min=32768):
    """(d2, nearest), uint32 each: one pass per obstacle, in ascending index order."""
    g = np.asarray(grid, np.uint16)
    rows, cols = g.shape
    rr, cc = np.mgrid[0:rows, 0:cols].astype(np.int64)
    d2 = np.full(g.shape, NONE, np.int64)
    nearest = np.full(g.shape, NONE, np.int64)
    for idx in np.flatnonzero(g.astype(np.int64).reshape(-1) >= occupied_min):      # ascending
        r, c = divmod(int(idx), cols)
        d = (rr - r) ** 2 + (cc - c) ** 2
        closer = d < d2                                                            # strict: the first index stays
        d2[closer] = d[closer]
        nearest[closer] = idx
    return d2.astype(np.uint32), nearest.astype(np.uint32)


def distance_map(grid, table, R, occupied_min=32768, keep_unknown=False, d2=None):
    """out(c) = T[min(d2(c), R^2)]; an unknown cell stays 0 under keep_unknown."""
    g = np.asarray(grid, np.uint16)
    if d2 is None:
        d2 = transform(g, occupied_min)[0]
    out = np.asarray(table, np.uint16)[np.minimum(d2.astype(np.int64), R * R)]
    if keep_unknown:
        out = np.where(g == 0, 0, out)
    return out.astype(np.uint16)


def first_known(grid):
    """(smallest row, smallest column) holding a non-zero cell; (rows, cols) if there is none."""
    g = np.asarray(grid)
    rr, cc = np.nonzero(g)
    return (int(rr.min()), int(cc.min())) if rr.size else (int(g.shape[0]), int(g.shape[1]))


# ---- the cases ----

def _random(shape, seed, density):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 32768, shape).astype(np.uint16)
    g[rng.random(shape) < 0.4] = 0                                       # unknown cells
    hit = rng.random(shape) < density
    g[hit] = rng.integers(32768, 65535, shape).astype(np.uint16)[hit]    # obstacles, <= 65534
    return g


def _with(shape, cells, fill=700, value=50000):
    g = np.full(shape, fill, np.uint16)
    for k, rc in enumerate(cells):
        g[rc] = value + k
    return g


CROSS = [(5, 0), (0, 5), (10, 5), (5, 10)]                  # all 5 from (5, 5): the smallest index is (0, 5) = 5
PYTHAGORAS = [(10, 5), (8, 9), (2, 1), (9, 2), (5, 10)]     # all 5 from (5, 5) on 12 x 12: the smallest is (2, 1) = 25
LAST_COLUMN = (63, 64, 65, 255, 256, 257)
DENSITIES = (0.002, 0.03, 0.5)
SEAM_SHAPES = ((37, 53), (65, 130), (97, 131))
FUZZ = 20


def _line(n, marks):
    g = np.where(np.arange(n) % 7 < 4, 700, 0).astype(np.uint16)
    for k, i in enumerate(marks):
        g[i] = 40000 + 1000 * k
    return g


def _max_value():
    g = _random((24, 40), 11, 0.05)
    g[7, 9] = 65535
    g[20, 33] = 65535
    return g


def _low_known():
    """random65x130 at 0.03 without its first 9 rows and 11 columns."""
    g = _random((65, 130), 3, 0.03).copy()
    g[:9, :] = 0
    g[:, :11] = 0
    g[10, 12] = 52000
    return g


def _fuzz(i):
    rng = np.random.default_rng(7000 + i)
    shape = (int(rng.integers(1, 97)), int(rng.integers(1, 97)))
    density = float(np.exp(rng.uniform(np.log(0.001), np.log(0.5))))
    return _random(shape, 7100 + i, density)


_GRIDS = {
    "one_cell": lambda: np.full((1, 1), 50000, np.uint16),
    "one_cell_free": lambda: np.full((1, 1), 900, np.uint16),
    "line1x200": lambda: _line(200, (0, 199, 63, 64, 65)).reshape(1, 200),
    "line200x1": lambda: _line(200, (0, 199, 63, 64, 65, 31, 32, 33)).reshape(200, 1),
    "no_obstacle": lambda: _random((20, 33), 4, 0.0),
    "all_obstacle": lambda: _random((20, 33), 4, 0.0) // 2 + np.uint16(40000),
    "max_value": _max_value,
    "cross": lambda: _with((11, 11), CROSS),
    "pythagoras": lambda: _with((12, 12), PYTHAGORAS),
    "tie_column": lambda: _with((9, 5), [(1, 2), (7, 2)]),          # (4, 2) is 3 from both
    "tie_row": lambda: _with((5, 9), [(2, 1), (2, 7)]),             # (2, 4) is 3 from both
    "own_row_tie": lambda: _with((11, 11), [(5, 2), (8, 3)]),       # (5, 7) is 5 from both; (5, 2) is in its row
    "tall_last_row": lambda: _with((4 * RUN_ROWS + 3, 9), [(4 * RUN_ROWS + 2, 4)]),
    "pad70": lambda: _random((13, 70), 21, 0.02),
    "pad130": lambda: _random((9, 130), 22, 0.02),
    "far200": lambda: _with((200, 200), [(199, 199)], fill=0),
    "clamp2x300": lambda: _with((2, 300), [(0, 0)]),
    "low_known": _low_known,
    # wider than WIDE_COLS: the row pass stages one row per trip and puts the whole workgroup on it
    "wide": lambda: _with((RUN_ROWS + 1, WIDE_COLS + 9), [(0, 0), (RUN_ROWS, WIDE_COLS + 8), (1, WIDE_COLS // 2)]),
    # the two shapes whose staged rows pass 64 KB of LDS, which the launch has to be granted: four rows of
    # WIDE_COLS columns, and one row of the largest width there is
    "wide_four_rows": lambda: _with((RUN_ROWS + 1, WIDE_COLS), [(0, 0), (RUN_ROWS, WIDE_COLS - 1), (2, 5000)]),
    "widest": lambda: _with((2, MAX_SIDE), [(0, 0), (1, MAX_SIDE - 1), (0, 16000)]),
    # the largest row offsets an int16 has to hold, downwards and upwards: -32766 and +32766
    "tallest_top": lambda: _with((MAX_SIDE, 1), [(0, 0)]),
    "tallest_bottom": lambda: _with((MAX_SIDE, 1), [(MAX_SIDE - 1, 0)]),
}
for _n in LAST_COLUMN:
    _GRIDS["last_column%d" % _n] = (lambda n: lambda: _with((RUN_ROWS + 2, n), [(0, n - 1), (RUN_ROWS, n - 1)]))(_n)
for _k, _shape in enumerate(SEAM_SHAPES):
    for _d in DENSITIES:
        _GRIDS["random%dx%d_%g" % (_shape + (_d,))] = (lambda s, k, d: lambda: _random(s, 30 + k, d))(_shape, _k, _d)
for _i in range(FUZZ):
    _GRIDS["fuzz%d" % _i] = (lambda i: lambda: _fuzz(i))(_i)

RANDOM_CASES = ["random%dx%d_%g" % (s + (d,)) for s in SEAM_SHAPES for d in DENSITIES]
FUZZ_CASES = ["fuzz%d" % i for i in range(FUZZ)]
# (grid name, occupied_min)
CASES = ([(n, 32768) for n in ("one_cell", "one_cell_free", "line1x200", "line200x1", "no_obstacle", "all_obstacle")]
         + [("max_value", 65535), ("max_value", 70000)]
         + [(n, 32768) for n in ("cross", "pythagoras", "tie_column", "tie_row", "own_row_tie", "tall_last_row", "pad70", "pad130",
                                 "far200", "clamp2x300", "low_known", "wide", "wide_four_rows", "widest", "tallest_top",
                                 "tallest_bottom")]
         + [("last_column%d" % n, 32768) for n in LAST_COLUMN]
         + [(n, 32768) for n in RANDOM_CASES + FUZZ_CASES])


@functools.lru_cache(maxsize=None)
def grid_of(name):
    g = _GRIDS[name]()
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def expected(name, occupied_min=32768):
    """(grid, d2, nearest) of a case; computed once per session."""
    g = grid_of(name)
    d2, nearest = transform(g, occupied_min)
    for a in (d2, nearest):
        a.setflags(write=False)
    return g, d2, nearest


def table_of(kind, R):
    """"gauss": kernel(sigma = R / 3 cells), floor 1; "cut": the same with T[R^2] = 0, so cells at R and beyond
    stay unknown; "ramp": 65534 - d2 mod 65533, a different value at every d2 and never 0; "zeros"."""
    if kind == "gauss":
        return kernel(R * RES / 3.0, RES, R)
    if kind == "cut":
        t = kernel(R * RES / 3.0, RES, R)
        t[R * R] = 0
        return t
    if kind == "ramp":
        return np.array([65534 - d2 % 65533 for d2 in range(R * R + 1)], np.uint16)
    if kind == "zeros":
        return np.zeros(R * R + 1, np.uint16)
    raise KeyError(kind)


CLAMP_RADII = (1, 2, 5, 16, 255)
# (grid name, R, table kind, occupied_min): the fields the GPU tests build
FIELD_CASES = ([(n, R, "ramp", m) for n, m in CASES if not n.startswith("fuzz") for R in (2, 16)]
               + [(n, 5, "gauss", 32768) for n in FUZZ_CASES]
               + [(n, R, "ramp", 32768) for n in ("far200", "clamp2x300") for R in CLAMP_RADII]
               + [("random37x53_0.03", R, "gauss", 32768) for R in CLAMP_RADII])


@functools.lru_cache(maxsize=None)
def field_expected(name, R, kind, occupied_min, keep_unknown):
    """(grid, table, reference field) of a FIELD_CASES entry; computed once per session."""
    g, d2, _ = expected(name, occupied_min)
    t = table_of(kind, R)
    out = distance_map(g, t, R, occupied_min, keep_unknown, d2)
    for a in (t, out):
        a.setflags(write=False)
    return g, t, out
