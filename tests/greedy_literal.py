"""Literal restatement of CostGreedyEndpoint::{Cost, ComputeGradient,
ComputeCovariance} (src/my_lidar_graph_slam/mapping/cost_function_greedy_endpoint.cpp)
and ScanMatcherHillClimbing::OptimizePose
(src/my_lidar_graph_slam/mapping/scan_matcher_hill_climbing.cpp:72-180),
statement by statement, independent of the library's cost code.

glibc for the transcendental functions (math.cos / math.sin / math.exp);
NumPy only for exactly rounded element-wise arithmetic, index arithmetic, cell
reads and threshold tests. Beam sums are taken in beam order (np.cumsum), never
with sum() (compensated since Python 3.12) or np.sum (pairwise). The probability
table and Compound / MoveBackward come from the library's host functions, which
tests/test_cpu_oracle.py and tests/test_cpu_host.py pin to the reference.
"""
import ctypes
import ctypes.util
import math

import numpy as np

from csm_hip import api

_PLUT = None

# Distance() is std::hypot, i.e. glibc's hypot; math.hypot has its own algorithm (Python >= 3.8)
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.hypot.restype = ctypes.c_double
_libm.hypot.argtypes = [ctypes.c_double, ctypes.c_double]


def hypot(x, y):
    return _libm.hypot(x, y)


def plut():
    global _PLUT
    if _PLUT is None:
        _PLUT = api.host_probability_lut()
    return _PLUT


DEFAULT_GREEDY = dict(map_resolution=0.05, hit_and_missed_dist=0.075, occupancy_threshold=0.1,
                      kernel_size=1, standard_deviation=0.05, scaling_factor=1.0)


class Greedy:
    """CostGreedyEndpoint(mapResolution, hitAndMissedDist, occupancyThreshold,
    kernelSize, scalingFactor, standardDeviation)."""

    def __init__(self, map_resolution, hit_and_missed_dist, occupancy_threshold, kernel_size,
                 standard_deviation, scaling_factor):
        self.res = map_resolution
        self.hmd = hit_and_missed_dist
        self.thr = occupancy_threshold
        self.k = kernel_size
        self.sd = standard_deviation
        self.var = standard_deviation * standard_deviation
        self.scale = scaling_factor
        self.setup_lookup_table()

    def setup_lookup_table(self):
        k = self.k
        size = 2 * k + 1
        self.lut = [0.0] * (size * size)
        for ky in range(-k, k + 1):
            for kx in range(-k, k + 1):
                diff_x = self.res * kx
                diff_y = self.res * ky
                sq = diff_x * diff_x + diff_y * diff_y
                self.lut[(k + ky) * size + (k + kx)] = -math.exp(-0.5 * sq / self.var)
        max_dx = self.res * (k + 1)
        max_dy = self.res * (k + 1)
        max_sq = max_dx * max_dx + max_dy * max_dy
        self.default = -math.exp(-0.5 * max_sq / self.var)

    def beam_values(self, grid, geom, angles, ranges, pose, alloc=None):
        """minCostValue of every beam (Cost's loop body), as a float64 array. alloc: None (every
        cell readable) or (bitmap, log2_block), the map's block allocation; a read in an
        unallocated block returns ProbabilityOr's default 0.0."""
        res, off_x, off_y = geom
        n = len(angles)
        cs = np.empty(n)
        sn = np.empty(n)
        for i in range(n):
            cs[i] = math.cos(pose[2] + float(angles[i]))
            sn[i] = math.sin(pose[2] + float(angles[i]))
        r = np.asarray(ranges, dtype=np.float64)
        # ScanData::HitAndMissedPoint
        hx = pose[0] + r * cs
        hy = pose[1] + r * sn
        rm = r - self.hmd
        mx = pose[0] + rm * cs
        my = pose[1] + rm * sn
        # GridMapGeometry::PositionToIndex
        hc = np.floor((hx - off_x) / res).astype(np.int64)
        hr = np.floor((hy - off_y) / res).astype(np.int64)
        mc = np.floor((mx - off_x) / res).astype(np.int64)
        mr = np.floor((my - off_y) / res).astype(np.int64)
        rows, cols = grid.shape
        pl = plut()

        def prob_or(row, col):
            inside = (row >= 0) & (row < rows) & (col >= 0) & (col < cols)
            if alloc is not None:
                bitmap, log2_block = alloc
                blk = np.zeros(row.shape, bool)
                blk[inside] = bitmap[row[inside] >> log2_block, col[inside] >> log2_block] != 0
                inside &= blk
            v = np.zeros(row.shape, np.uint16)
            v[inside] = grid[row[inside], col[inside]]
            return np.where(inside, pl[v], 0.0)

        best = np.full(n, self.default)
        k, size = self.k, 2 * self.k + 1
        for ky in range(-k, k + 1):
            for kx in range(-k, k + 1):
                hp = prob_or(hr + ky, hc + kx)
                mp = prob_or(mr + ky, mc + kx)
                keep = ~((hp == 0.0) | (mp == 0.0)) & ~((hp < self.thr) | (mp > self.thr))
                cost = self.lut[(k + ky) * size + (k + kx)]
                best = np.where(keep, np.minimum(best, cost), best)
        return best

    def cost(self, grid, geom, angles, ranges, pose, alloc=None):
        vals = self.beam_values(grid, geom, angles, ranges, pose, alloc)
        s = float(np.cumsum(vals)[-1])      # sumCostValue += minCostValue, in beam order
        s *= self.scale
        return s

    def gradient(self, grid, geom, angles, ranges, pose, alloc=None):
        diff_linear = geom[0]
        diff_angular = 1e-2

        def c(p):
            return self.cost(grid, geom, angles, ranges, p, alloc)
        x, y, t = pose
        dx = c((x + diff_linear, y + 0.0, t + 0.0)) - c((x - diff_linear, y - 0.0, t - 0.0))
        dy = c((x + 0.0, y + diff_linear, t + 0.0)) - c((x - 0.0, y - diff_linear, t - 0.0))
        dt = c((x + 0.0, y + 0.0, t + diff_angular)) - c((x - 0.0, y - 0.0, t - diff_angular))
        return (0.5 * dx / diff_linear, 0.5 * dy / diff_linear, 0.5 * dt / diff_angular)

    def covariance(self, grid, geom, angles, ranges, pose, alloc=None):
        g = self.gradient(grid, geom, angles, ranges, pose, alloc)
        cov = [[g[i] * g[j] for j in range(3)] for i in range(3)]
        cov[0][0] += 0.1
        cov[1][1] += 0.1
        cov[2][2] += 0.1
        return np.array(cov)


def optimize_pose(grid, geom, angles, ranges, rel_pose, init_pose, linear_step, angular_step,
                  max_iterations, max_refinements, greedy, alloc=None):
    """ScanMatcherHillClimbing::OptimizePose; returns the summary fields and metrics.
    alloc: the map's block allocation, as in Greedy.beam_values."""
    move_x = (1.0, -1.0, 0.0, 0.0, 0.0, 0.0)
    move_y = (0.0, 0.0, 1.0, -1.0, 0.0, 0.0)
    move_t = (0.0, 0.0, 0.0, 0.0, 1.0, -1.0)
    cf = greedy if isinstance(greedy, Greedy) else Greedy(**{**DEFAULT_GREEDY, **(greedy or {})})
    n = len(angles)
    sensor = tuple(api.host_compound(init_pose, rel_pose))
    initial_cost = cf.cost(grid, geom, angles, ranges, sensor, alloc)
    normalized_initial = initial_cost / n
    min_cost = initial_cost
    best = sensor
    iterations = 0
    refinements = 0
    lin, ang = linear_step, angular_step
    while True:
        min_local = min_cost
        best_local = best
        updated = False
        for i in range(6):
            pose = (best[0] + move_x[i] * lin, best[1] + move_y[i] * lin, best[2] + move_t[i] * ang)
            c = cf.cost(grid, geom, angles, ranges, pose, alloc)
            if c < min_local:
                min_local = c
                best_local = pose
                updated = True
        if updated:
            min_cost = min_local
            best = best_local
        else:
            refinements += 1
            lin *= 0.5
            ang *= 0.5
        # (poseUpdated || numOfRefinements < Max) && (++numOfIterations < MaxIterations)
        if not (updated or refinements < max_refinements):
            break
        iterations += 1
        if not iterations < max_iterations:
            break
    estimated = tuple(api.host_move_backward(best, rel_pose))
    cov = cf.covariance(grid, geom, angles, ranges, best, alloc)
    return dict(normalized_initial_cost=normalized_initial, normalized_cost=min_cost / n,
                sensor_pose=list(sensor), best_sensor_pose=list(best), estimated_pose=list(estimated),
                covariance=cov, iterations=iterations, refinements=refinements,
                diff_translation=hypot(init_pose[0] - estimated[0], init_pose[1] - estimated[1]),
                diff_rotation=abs(init_pose[2] - estimated[2]))
