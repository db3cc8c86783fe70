"""Pose sets (include/csm_hip.h, csm_score_pose_sets and csm_pose_set_update) restated literally: the records
in numpy over the oracle's own projection (oracle.project: HitPoint + PositionToIndex at one sensor pose), the
weights and ancestors in plain integer Python. Also the seeded maps, scans and poses that
tests/test_cpu_pose_sets.py, tests/test_gpu_pose_sets.py and tests/test_gpu_pose_sets_adapter.py share, and the
certificate's margin in numpy (how many poses of a case the device will hand to the host)."""
import bisect
import itertools

import numpy as np

from csm_hip import api
from oracle import oracle as O

VOLUME_BINS = 1024
ROWS, COLS = 48, 64                  # non-square, so a row / column swap shows
GEOM = (0.05, -1.6, -1.2)            # x in [-1.6, 1.6), y in [-1.2, 1.2)


def make_map(seed, rows=ROWS, cols=COLS, known=0.6):
    """A grid of raw values, about `known` of the cells known (non-zero)."""
    rng = np.random.RandomState(seed)
    grid = rng.randint(1, 65536, size=(rows, cols)).astype(np.uint16)
    grid[rng.uniform(size=(rows, cols)) > known] = 0
    return grid


def make_scan(seed, n_points, r_lo=0.2, r_hi=1.5):
    rng = np.random.RandomState(1000 + seed)
    angles = -np.pi + 2.0 * np.pi * np.arange(n_points) / n_points + rng.uniform(-1e-3, 1e-3, n_points)
    return angles, rng.uniform(r_lo, r_hi, n_points)


def make_poses(seed, n_poses, half_x=1.0, half_y=0.8, centre=(0.0, 0.0)):
    rng = np.random.RandomState(2000 + seed)
    return np.stack([centre[0] + rng.uniform(-half_x, half_x, n_poses),
                     centre[1] + rng.uniform(-half_y, half_y, n_poses),
                     rng.uniform(-np.pi, np.pi, n_poses)], axis=1).reshape(-1, 3)


def score_poses(grid, geom, angles, ranges, poses):
    """(S, K) per pose: the sum of the raw values of the known hit cells inside the map, and their count."""
    grid = np.asarray(grid)
    rows, cols = grid.shape
    S, K = [], []
    for pose in np.asarray(poses, dtype=np.float64).reshape(-1, 3):
        col, row = O.project(geom, pose, angles, ranges)
        inside = (col >= 0) & (col < cols) & (row >= 0) & (row < rows)
        v = grid[row[inside], col[inside]].astype(np.int64)
        S.append(int(v.sum()))
        K.append(int((v != 0).sum()))
    return np.array(S, dtype=np.int64), np.array(K, dtype=np.int64)


def records_sk(records):
    return records["sum_values"].astype(np.int64), records["known"].astype(np.int64)


def key(s, k):
    return 32268 * int(k) + 499 * int(s)


def min_known(n_points, threshold):
    return min([j for j in range(n_points + 2) if j / n_points > threshold] + [n_points + 1])


def update(S, K, n_points, temperature, threshold=0.0, n_out=None, offset=0):
    """(weights, ancestors, info) of the definition, Python integers throughout; the table is the volume
    covariance's (csm_host_volume_weights, checked by its own tests)."""
    table, shift = api.host_volume_weights(n_points, temperature)
    table = [int(w) for w in table]
    n = len(S)
    n_out = n if n_out is None else n_out
    need = min_known(n_points, threshold)
    keys = [key(s, k) for s, k in zip(S, K)]
    eligible = [int(k) >= need for k in K]
    info = dict(m0=0, key_max=0, best_index=-1, support=0, bin_shift=shift, found=0)
    if any(eligible):
        info["key_max"] = max(kk for kk, e in zip(keys, eligible) if e)
        info["best_index"] = next(i for i in range(n) if eligible[i] and keys[i] == info["key_max"])
        info["found"] = 1
    weights = []
    for i in range(n):
        w = 0
        if info["found"] and eligible[i]:
            b = (info["key_max"] - keys[i]) >> shift
            w = table[b] if b < VOLUME_BINS else 0
        weights.append(w)
    info["m0"] = sum(weights)
    info["support"] = sum(1 for w in weights if w > 0)
    prefix, c = [], 0
    for w in weights:
        c += w
        prefix.append(c)
    ancestors = []
    for j in range(n_out):
        if not info["found"]:
            ancestors.append(-1)
            continue
        t = (j * info["m0"] + offset % info["m0"]) // n_out
        ancestors.append(next(i for i in range(n) if prefix[i] > t))
    return weights, ancestors, info


def update_fast(S, K, n_points, temperature, threshold=0.0, n_out=None, offset=0):
    """update() for sets too large for its quadratic searches (2^18 poses, 2^18 outputs): the same result from
    one pass for the maximum, itertools.accumulate for the prefix and bisect_right for the ancestors (the
    smallest i with prefix[i] > t). Python integers throughout; tests/test_cpu_pose_sets_cases.py pins it to
    update(), which stays the definition."""
    table, shift = api.host_volume_weights(n_points, temperature)
    table = [int(w) for w in table]
    n = len(S)
    n_out = n if n_out is None else n_out
    need = min_known(n_points, threshold)
    keys = [32268 * int(k) + 499 * int(s) for s, k in zip(S, K)]
    eligible = [int(k) >= need for k in K]
    info = dict(m0=0, key_max=0, best_index=-1, support=0, bin_shift=shift, found=0)
    for i in range(n):                                   # strict >: the first holder of the maximum stays
        if eligible[i] and (not info["found"] or keys[i] > info["key_max"]):
            info["key_max"], info["best_index"], info["found"] = keys[i], i, 1
    weights = [0] * n
    if info["found"]:
        for i in range(n):
            if eligible[i]:
                b = (info["key_max"] - keys[i]) >> shift
                weights[i] = table[b] if b < VOLUME_BINS else 0
    prefix = list(itertools.accumulate(weights))
    info["m0"] = prefix[-1] if n else 0
    info["support"] = sum(1 for w in weights if w > 0)
    if not info["found"]:
        return weights, [-1] * n_out, info
    m0, u = info["m0"], offset % info["m0"]
    return weights, [bisect.bisect_right(prefix, (j * m0 + u) // n_out) for j in range(n_out)], info


def margin_uncertain(geom, angles, ranges, poses):
    """Per pose: would the device mark it? The certificate of k_pose_score evaluated in numpy f64 (numpy's
    sin / cos stand in for the device's: a beam's distance from a cell edge moves by far less than the margin
    it is compared with, so the count is the device's up to beams within a few ulp of the margin itself)."""
    res, off_x, off_y = geom
    a, r = np.asarray(angles, np.float64), np.asarray(ranges, np.float64)
    poses = np.asarray(poses, np.float64).reshape(-1, 3)
    inv = 1.0 / res
    out = np.zeros(poses.shape[0], bool)
    for p, (x, y, th) in enumerate(poses):
        trig = 2.4e-15 + 4e-16 * (abs(th) + np.abs(a).max())
        hx = x + r * (np.cos(th) * np.cos(a) - np.sin(th) * np.sin(a))
        hy = y + r * (np.sin(th) * np.cos(a) + np.cos(th) * np.sin(a))
        bad = np.zeros(a.size, bool)
        for h, off in ((hx, off_x), (hy, off_y)):
            q = (h - off) * inv
            f = q - np.floor(q)
            m = 64.0 * ((np.abs(r) * trig + (np.abs(h) + abs(off)) * 4e-16) * inv + np.abs(q) * 8e-16)
            bad |= ~((f > m) & (f < 1.0 - m))
        out[p] = bad.any()
    return out


# the basic sweep of the GPU tests: every beam count with every pose count, on make_map(1)
SWEEP_POINTS = (1, 63, 64, 65, 360)
SWEEP_POSES = (1, 63, 64, 65, 257, 1000)


def sweep_case(n_points, n_poses):
    angles, ranges = make_scan(n_points, n_points)
    return dict(geom=GEOM, angles=angles, ranges=ranges, poses=make_poses(n_points * 7 + n_poses, n_poses))


def edge_case():
    """The forced uncertified pose: resolution 2^-4, dyadic offsets, a beam at angle 0 whose hit point
    x + r = 0.75 lies exactly on a cell edge ((0.75 + 2) / 0.0625 = 44). Pose 1 is in general position."""
    geom = (0.0625, -2.0, -1.5)
    angles = np.array([0.0, 0.7, -1.9, 2.6])
    ranges = np.array([0.5, 0.8, 0.6, 1.1])
    poses = np.array([[0.25, 0.031, 0.0], [0.13, -0.21, 0.4]])
    return dict(geom=geom, angles=angles, ranges=ranges, poses=poses)
