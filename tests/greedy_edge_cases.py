"""Inputs of the greedy-endpoint / hill-climbing parity tests that the CPU suite
(tests/test_cpu_greedy.py) and the GPU suite (tests/test_gpu_greedy_edges.py) share: the settings
sweep, maps ringed with known cells, the scans that put a coordinate exactly on a cell edge, and
the reads of the kernel windows. Pure numpy + synth; no GPU."""
import math

import numpy as np

from csm_hip import synth
import greedy_literal as GL


class PlutAt:
    """An occupancy threshold equal to the probability of cell value v, resolved when used."""

    def __init__(self, v):
        self.v = v

    def __repr__(self):
        return "PlutAt(%d)" % self.v


def settings(overrides):
    """CostGreedyEndpoint settings: the defaults with `overrides`, thresholds resolved."""
    out = {**GL.DEFAULT_GREEDY, **overrides}
    if isinstance(out["occupancy_threshold"], PlutAt):
        out["occupancy_threshold"] = float(GL.plut()[out["occupancy_threshold"].v])
    return out


V_EQ = 20000                 # a value planted under both hit and missed points, and the threshold
# exp(-0.5 res^2 / sd^2) with an exponent of -720 at one cell (res 0.05): a denormal; from two
# cells on, and for the default, it underflows to 0 (LUT entries -0.0)
SD_DENORMAL = math.sqrt(0.5 * 0.05 * 0.05 / 720.0)


def case(seed, n_beams=180, unknown=False, off_map=False, res=0.05, plant=None):
    """One scan over a 200 x 220 room. plant: a cell value written into 40 % of the known cells
    (walls and free space alike)."""
    c = synth.csm_case(seed, rows=200, cols=220, res=res, n_beams=n_beams, fov=1.5 * math.pi,
                       max_range=4.0, rel_pose=(0.05, -0.02, 0.01))
    grid = c["grid"].copy()
    if unknown:
        grid[60:140, :90] = 0            # an unknown region under part of the scan
    if plant is not None:
        rng = np.random.RandomState(seed)
        grid[(grid > 0) & (rng.rand(*grid.shape) < 0.4)] = plant
    init = tuple(c["init_pose"])
    if off_map == "partly":
        init = (init[0] + 0.45 * grid.shape[1] * res, init[1], init[2])
    elif off_map == "wholly":
        init = (init[0] + 40.0, init[1] - 40.0, init[2])
    return grid, c, init


CASES = [
    # (seed, greedy overrides, hill-climbing settings, case options)
    (1, dict(kernel_size=0), (0.1, 0.1, 100, 5), {}),
    (2, dict(kernel_size=1), (0.1, 0.1, 100, 5), {}),
    (3, dict(kernel_size=2), (0.1, 0.1, 100, 5), {}),
    (4, dict(kernel_size=3), (0.05, 0.05, 30, 3), {}),
    (5, dict(occupancy_threshold=0.6), (0.1, 0.1, 100, 5), {}),
    (6, dict(occupancy_threshold=0.6, kernel_size=2), (0.01, 0.01, 5, 2), {}),
    (7, dict(scaling_factor=2.5), (0.1, 0.1, 100, 5), {}),
    (8, dict(scaling_factor=-1.0), (0.1, 0.1, 20, 5), {}),
    (9, dict(map_resolution=0.03), (0.1, 0.1, 100, 5), {}),
    (10, dict(map_resolution=0.08, kernel_size=2), (0.01, 0.01, 5, 2), {}),
    (11, {}, (0.1, 0.1, 100, 5), dict(off_map="partly")),
    (12, {}, (0.1, 0.1, 100, 5), dict(off_map="wholly")),
    (13, {}, (0.1, 0.1, 100, 5), dict(unknown=True)),
    (14, dict(kernel_size=2), (0.1, 0.1, 1, 5), {}),
    (15, {}, (0.1, 0.1, 100, 0), {}),
    (16, {}, (0.01, 0.01, 5, 2), {}),
    (17, dict(hit_and_missed_dist=0.15, standard_deviation=0.1), (0.1, 0.1, 100, 5), {}),
    (18, {}, (0.1, 0.1, 100, 5), dict(res=0.04)),
    (19, dict(scaling_factor=2.5, kernel_size=0), (0.05, 0.1, 40, 1), dict(unknown=True)),
    (20, dict(kernel_size=1), (0.1, 0.1, 100, 5), dict(n_beams=2)),
    # large kernels (the literal walks (2k+1)^2 offsets: short searches, few beams)
    (21, dict(kernel_size=4), (0.05, 0.05, 6, 1), dict(n_beams=90)),
    (22, dict(kernel_size=5), (0.05, 0.05, 4, 1), dict(n_beams=90)),
    (23, dict(kernel_size=8), (0.05, 0.05, 3, 1), dict(n_beams=60)),
    # thresholds equal to a value the map holds under hit and missed points; below plut[1]; at
    # plut[65535] (only that value passes as a hit) and above it (nothing does)
    (24, dict(occupancy_threshold=PlutAt(V_EQ), kernel_size=0), (0.1, 0.1, 100, 5), dict(plant=V_EQ)),
    (25, dict(occupancy_threshold=PlutAt(V_EQ), kernel_size=1), (0.1, 0.1, 100, 5), dict(plant=V_EQ)),
    (26, dict(occupancy_threshold=5e-4), (0.1, 0.1, 100, 5), {}),
    (27, dict(occupancy_threshold=PlutAt(65535)), (0.1, 0.1, 100, 5), dict(plant=65535)),
    (28, dict(occupancy_threshold=1.0), (0.1, 0.1, 100, 5), {}),
    # LUT entries that are denormal or -0.0
    (29, dict(standard_deviation=SD_DENORMAL, kernel_size=2), (0.1, 0.1, 100, 5), {}),
    (30, dict(standard_deviation=SD_DENORMAL, kernel_size=1), (0.1, 0.1, 100, 5), dict(unknown=True)),
    # a single distinct value
    (31, dict(map_resolution=0.0), (0.1, 0.1, 100, 5), {}),
    # missed points behind the sensor; in front of the hit point
    (32, dict(hit_and_missed_dist=1.5), (0.1, 0.1, 100, 5), {}),
    (33, dict(hit_and_missed_dist=-0.1), (0.1, 0.1, 100, 5), {}),
    (34, dict(scaling_factor=0.0), (0.1, 0.1, 100, 5), {}),
    (35, {}, (0.1, 0.1, 1, 0), {}),
    # costs that overflow to -inf (covariance NaN); with two beams, finite and -inf costs mix
    (36, dict(scaling_factor=1e308), (0.1, 0.1, 100, 5), {}),
    (37, dict(scaling_factor=1e308), (0.1, 0.1, 100, 5), dict(n_beams=2)),
]


# ---------------------------------------------------------------- map edges


def ringed(grid, seed):
    """The room with known cells of any value along the whole map border, so that kernel windows
    across an edge read known cells on the inside."""
    g = grid.copy()
    rng = np.random.RandomState(seed)
    for sl in ((slice(0, 2), slice(None)), (slice(-2, None), slice(None)),
               (slice(None), slice(0, 2)), (slice(None), slice(-2, None))):
        g[sl] = rng.randint(1, 65536, size=g[sl].shape)
    return g


def cell_indices(geom, pose, angles, ranges, hmd):
    """PositionToIndex of the hit and missed points, as the literal computes them."""
    res, ox, oy = geom
    a = pose[2] + np.asarray(angles, np.float64)
    c = np.array([math.cos(v) for v in a])
    s = np.array([math.sin(v) for v in a])
    r = np.asarray(ranges, np.float64)
    out = {}
    for name, rr in (("hit", r), ("missed", r - hmd)):
        out[name] = (np.floor((pose[0] + rr * c - ox) / res).astype(np.int64),
                     np.floor((pose[1] + rr * s - oy) / res).astype(np.int64))
    return out


def straddles(geom, shape, pose, angles, ranges, k, hmd):
    """Per point kind and map side: how many kernel windows [col - k, col + k] x [row - k, row + k]
    hold cells on both sides of that edge of the map, with some of them inside it."""
    rows, cols = shape
    out = {}
    for kind, (col, row) in cell_indices(geom, pose, angles, ranges, hmd).items():
        rows_in = (row + k >= 0) & (row - k < rows)
        cols_in = (col + k >= 0) & (col - k < cols)
        out[kind] = dict(left=int(((col - k < 0) & (col + k >= 0) & rows_in).sum()),
                         right=int(((col - k < cols) & (col + k >= cols) & rows_in).sum()),
                         below=int(((row - k < 0) & (row + k >= 0) & cols_in).sum()),
                         above=int(((row - k < rows) & (row + k >= rows) & cols_in).sum()))
    return out


def window_reads(grid, alloc, log2_block, geom, pose, angles, ranges, k, hmd):
    """Reads of the kernel windows inside the map: (in unallocated blocks, of unknown cells in
    allocated ones)."""
    rows, cols = grid.shape
    unalloc = unknown = 0
    for col, row in cell_indices(geom, pose, angles, ranges, hmd).values():
        for ky in range(-k, k + 1):
            for kx in range(-k, k + 1):
                r, c = row + ky, col + kx
                inside = (r >= 0) & (r < rows) & (c >= 0) & (c < cols)
                r, c = r[inside], c[inside]
                blk = alloc[r >> log2_block, c >> log2_block] != 0
                unalloc += int((~blk).sum())
                unknown += int((blk & (grid[r, c] == 0)).sum())
    return unalloc, unknown


# ---------------------------------------------------------------- points on cell edges

EDGE_RES = 0.0625             # exact in binary: x + r - off_x and its quotient are exact
EDGE_OFF = (-8.0, -8.0)
EDGE_STEP = 0.03125           # linear step of the mid-search case: one half cell


def edge_map(seed):
    grid, _, segs = synth.make_room(seed, 256, 256, EDGE_RES)
    return grid, (EDGE_RES,) + EDGE_OFF, segs


def edge_scan(segs, pose, n_beams):
    """A scan from `pose` (theta 0) whose beam 0 points along +x (angle 0.0) with range 2.5: its hit
    x coordinate is pose x + 2.5. The other beams are cast at the room."""
    angles, ranges = synth.cast_scan(segs, pose, n_beams, 1.5 * math.pi, 5.0)
    angles, ranges = angles.copy(), ranges.copy()
    angles[0], ranges[0] = 0.0, 2.5
    return angles, ranges


def start_on_edge():
    """(a): the start pose puts beam 0's hit x exactly on a cell edge."""
    x, y = 1.25, 0.3
    q = (x + 2.5 * math.cos(0.0 + 0.0) - EDGE_OFF[0]) / EDGE_RES
    assert q == 188.0
    return (x, y, 0.0)


def first_move_on_edge():
    """(b): the start pose is half a cell off the edge; its first +x candidate (x + step) is on it."""
    x, y = 1.28125, 0.3
    q0 = (x + 2.5 * math.cos(0.0) - EDGE_OFF[0]) / EDGE_RES
    q1 = ((x + 1.0 * EDGE_STEP) + 2.5 * math.cos(0.0) - EDGE_OFF[0]) / EDGE_RES
    assert q0 == 188.5 and q1 == 189.0
    return (x, y, 0.0)
