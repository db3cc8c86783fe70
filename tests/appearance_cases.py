"""Seeded cases for the appearance tests: ragged scans, descriptor sets, and pose graphs built the way
loop_search_cases builds its own (its _finish: runs, map index and the literal travel accumulation).

  ragged(sizes)        scans of the given beam counts; angles a little beyond [-pi, pi), ranges a little beyond
                       [range_min, range_max), every 17th beam NaN or inf in one of its two values.
  descriptor_set(...)  n descriptors of small counts with a few saturated cells; the second half revisits the
                       first: node i + n/2 is node i rolled along the sector axis by a known shift, with a few
                       cells changed, so small distances at non-zero shifts exist between different maps.
  line_graph(n)        n nodes 0.25 m apart on a line (travel = 0.25 i exactly), maps of 1 to 13 nodes.
  scene_scans(...)     scans of one polygonal room seen from nodes with different headings (for the adapters).
"""
import functools

import numpy as np

import loop_search_cases as LC

SHAPES = ((1, 4), (3, 12), (20, 60), (20, 64), (32, 128))
RANGE_MIN, RANGE_MAX = 0.5, 20.0


def ragged(sizes, seed=5):
    rng = np.random.default_rng(seed)
    total = int(np.sum(sizes))
    angles = rng.uniform(-np.pi - 0.05, np.pi + 0.05, total)
    ranges = rng.uniform(RANGE_MIN - 0.3, RANGE_MAX + 0.3, total)
    bad = np.arange(total)[::17]
    for j, b in enumerate(bad):
        (angles if j % 2 else ranges)[b] = (np.nan, np.inf, -np.inf)[j % 3]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return angles, ranges, offsets


@functools.lru_cache(maxsize=None)
def descriptor_set(n, n_rings, n_sectors, seed=3):
    rng = np.random.default_rng(seed + 1000 * n_rings + n_sectors)
    d = rng.integers(0, 4, (n, n_rings, n_sectors)).astype(np.uint8)
    d[rng.random(d.shape) < 0.01] = 255
    half = n // 2
    shifts = rng.integers(0, n_sectors, n)
    for i in range(half, n):
        d[i] = np.roll(d[i - half], int(shifts[i]), axis=1)
        flip = rng.random(d[i].shape) < 0.02
        d[i][flip] = rng.integers(0, 6, int(flip.sum()))
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def line_graph(n):
    poses = np.zeros((n, 3))
    poses[:, 0] = 0.25 * np.arange(n)
    sizes = []
    while sum(sizes) < n:
        sizes.append(min(1 + (5 * len(sizes)) % 13, n - sum(sizes)))
    c = LC._finish(poses, sizes, 10.0, 2.0)
    assert np.array_equal(c["travel"], 0.25 * np.arange(n))
    return c


def search_case(n, n_rings, n_sectors, seed=3):
    """A line graph of n nodes with a descriptor per node."""
    c = dict(line_graph(n))
    c["desc"] = descriptor_set(n, n_rings, n_sectors, seed)
    return c


def _room_ranges(angles, pose, walls):
    """Distance along each beam from pose (x, y, theta) to the nearest of the wall segments."""
    out = np.full(len(angles), np.inf)
    ox, oy = pose[0], pose[1]
    dx, dy = np.cos(angles + pose[2]), np.sin(angles + pose[2])
    for (ax, ay), (bx, by) in walls:
        ex, ey = bx - ax, by - ay
        den = dx * ey - dy * ex
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((ax - ox) * ey - (ay - oy) * ex) / den
            u = ((ax - ox) * dy - (ay - oy) * dx) / den
        hit = (np.abs(den) > 1e-12) & (t > 0) & (u >= 0) & (u <= 1)
        out = np.where(hit & (t < out), t, out)
    return out


@functools.lru_cache(maxsize=None)
def scene(n_beams=360):
    """A pose graph of 60 nodes that walks through an L-shaped room twice with different headings, maps of
    10 nodes; scans[i] = (angles, ranges) of node i. Returns (graph dict, scans)."""
    corners = [(0, 0), (12, 0), (12, 5), (7, 5), (7, 9), (0, 9)]
    walls = [(corners[i], corners[(i + 1) % len(corners)]) for i in range(len(corners))]
    angles = -np.pi + 2.0 * np.pi * (np.arange(n_beams) + 0.5) / n_beams
    lap = [(1.0 + 0.3 * i, 2.0 + 0.05 * i) for i in range(30)]
    poses = np.array([(x, y, 0.1 * i) for i, (x, y) in enumerate(lap)] +
                     [(x + 0.05, y - 0.03, 2.0 + 0.07 * i) for i, (x, y) in enumerate(lap)])
    c = LC._finish(poses, [10] * 6, 5.0, 2.0)
    scans = tuple((angles, _room_ranges(angles, p, walls)) for p in poses)
    return c, scans
