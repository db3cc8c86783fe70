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
