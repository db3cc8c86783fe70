"""The inputs of tests/test_gpu_adapter_residency.py: two grids A and B of one shape under one geometry and
one scan, cast in A's room. The C++ adapters are asked the same question about A and about B under the same
map id; which of the two rows comes back says which cells the device held. No GPU is touched here:
tests/test_cpu_adapter_residency_cases.py proves on the CPU that the two rows differ for every matcher.

Small on purpose: a 200 x 200 map, 180 beams, an 11 x 11 x 11 grid search."""
import math

import numpy as np

from csm_hip import api, synth

ROWS = COLS = 200
N_BEAMS = 180
ID = 7                                                  # the caller's map id in the driver
GRID_SEARCH = (0.5, 0.5, 0.1, 0.05, 0.05, 0.01)         # ranges, steps: ceil(0.5 range / step) = 5 each way
HILL = (0.1, 0.1, 100, 5)                               # "ScanMatcherHillClimbing"
GREEDY = dict(map_resolution=0.05, hit_and_missed_dist=0.075, occupancy_threshold=0.1, kernel_size=1,
              standard_deviation=0.05, scaling_factor=1.0)              # "CostGreedyEndpoint"
CSM = (0.6, 0.6, math.radians(6), 4)                    # ranges, low resolution
PEAKS = (3, (2, 2, 1))                                  # K, exclusion half-widths
TAU = 0.02
BNB = (1.0, 1.0, 0.2, 2, 0.3, 0.5)                      # ranges, node height, thresholds
LDC = (1.0, 1.0, 0.2, 4, 0.3, 0.5)                      # ranges, low resolution, thresholds
MAP_NODE_POSE = (1.5, -0.7, 0.3)                        # global pose of the reference local map's node
_CASE = {}


def case():
    """dict(A, B, geom, angles, ranges, rel_pose, init_pose): built once, the grids read-only."""
    if not _CASE:
        c = synth.csm_case(4100, rows=ROWS, cols=COLS, n_beams=N_BEAMS, rel_pose=(0.04, -0.02, 0.01))
        b, _, _ = synth.make_room(4101, ROWS, COLS, 0.05)
        a = np.ascontiguousarray(c["grid"], np.uint16)
        b = np.ascontiguousarray(b, np.uint16)
        a.setflags(write=False)
        b.setflags(write=False)
        _CASE.update(A=a, B=b, geom=c["geom"], angles=c["angles"], ranges=c["ranges"], rel_pose=c["rel_pose"],
                     init_pose=c["init_pose"])
    return _CASE


def on(grid):
    """The case as the oracle and the host restatements take it, on `grid`."""
    c = case()
    return dict(grid=grid, geom=c["geom"], angles=c["angles"], ranges=c["ranges"], rel_pose=c["rel_pose"],
                init_pose=c["init_pose"])


def scan_node_global_pose():
    """The query scan node's global pose: the map node's pose compounded with the initial pose."""
    return tuple(api.host_compound(MAP_NODE_POSE, case()["init_pose"]))


def detector_init_pose():
    """What the detectors make of the two global poses (InverseCompound, loop_detector_branch_bound.cpp:
    97-98): the initial pose again, up to rounding."""
    return tuple(api.host_inverse_compound(MAP_NODE_POSE, scan_node_global_pose()))
