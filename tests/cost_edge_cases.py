"""Inputs of tests/test_gpu_cost_edges.py that the CPU suite checks too (tests/test_cpu_map_oracle.py):
device-built maps replayed on the oracle with the reference's block allocation tracked beside the
cells, and the decision margins of the linear solver. Pure numpy + the oracle; no GPU."""
import math

import numpy as np

from csm_hip import synth

REL_COST = 1e-10        # include/csm_hip.h: costs and Hessian entries (relative)
MARGIN = 1e3 * REL_COST  # a decision the two sides must take alike lies this far (relative) from its edge


def initial_shape(res, log2_block):
    """The fresh 1 m x 1 m map the reference starts from (grid_map_builder.cpp:80), on blocks
    of 2^log2_block cells."""
    bs = 1 << log2_block
    n = -(-int(math.ceil(1.0 / res)) // bs) * bs
    return dict(res=res, off_x=0.0, off_y=0.0, rows=n, cols=n, log2_block=log2_block)


def map_local(map_pose, pose, err=(0.0, 0.0, 0.0)):
    c, s = math.cos(map_pose[2]), math.sin(map_pose[2])
    dx, dy = pose[0] + err[0] - map_pose[0], pose[1] + err[1] - map_pose[1]
    return (c * dx + s * dy, -s * dx + c * dy, pose[2] + err[2] - map_pose[2])


def geom_of(shape):
    return (shape["res"], shape["off_x"], shape["off_y"])


def decision_margin(trace, iterations_max, threshold):
    """Smallest distance of a decision of ScanMatcherLinearSolver::OptimizePose from its edge, over
    the oracle's trace [(cost before, cost after, lambda)]: the stop test |change| < threshold
    (where it is evaluated: not after the last allowed iteration) and the damping update
    cost < previous cost (after every iteration but the last)."""
    m = math.inf
    for k, (prev, cost, _) in enumerate(trace):
        if k + 1 < iterations_max:
            m = min(m, abs(abs(prev - cost) - threshold))
        if k + 1 < len(trace):
            m = min(m, abs(prev - cost))
    return m


def margin_ok(trace, iterations_max, threshold):
    scale = max(max(p, c) for p, c, _ in trace)
    return decision_margin(trace, iterations_max, threshold) >= MARGIN * scale


def frontend_frames(oracle, log2_block, seed=77, n_scans=26):
    """The frontend loop of test_gpu_map_build.py::test_frontend_loop_over_a_trajectory: frame k
    rebuilds the latest map from the last 10 scan nodes in the frame the previous build left, then
    the new scan is matched against it. Yields per frame: the nodes and map pose of the build, the
    map's shape before and after, its cells and tracked allocation, and the query (the new scan at
    the oracle's correlative estimate, which the device matcher reproduces bit for bit)."""
    case = synth.map_case(seed, n_scans=n_scans, n_beams=360, step=0.15)
    nodes = case["nodes"]
    shape, alloc = initial_shape(0.05, log2_block), None
    for k in range(1, n_scans):
        window = nodes[max(0, k - 10):k]
        map_pose = window[0]["pose"]
        before = shape
        shape, grid, stats = oracle.construct_map(shape, map_pose, window, alloc=alloc)
        alloc = stats["alloc"]
        new = nodes[k]
        init = map_local(map_pose, new["pose"], (0.04, -0.03, 0.01))
        geom = geom_of(shape)
        found = oracle.csm(dict(grid=grid, geom=geom, angles=new["angles"], ranges=new["ranges"],
                                rel_pose=new["rel_pose"], init_pose=init), 0.5, 0.5, 0.2, 4)
        query = dict(geom=geom, angles=new["angles"], ranges=new["ranges"], rel_pose=new["rel_pose"],
                     init_pose=tuple(found["estimatedPose"]))
        yield dict(k=k, window=window, map_pose=map_pose, before=before, shape=shape, grid=grid, alloc=alloc,
                   query=query)


def fresh_construct(oracle, log2_block, seed=31):
    """A map built from the first 10 scans of a trajectory into a fresh id, and queries from the
    6 scans after them (they see parts of the room the map does not hold)."""
    case = synth.map_case(seed, n_scans=16, n_beams=720, step=0.15)
    nodes = case["nodes"]
    map_pose = nodes[0]["pose"]
    shape0 = initial_shape(0.05, log2_block)
    shape, grid, stats = oracle.construct_map(shape0, map_pose, nodes[:10])
    queries = [dict(geom=geom_of(shape), angles=nd["angles"], ranges=nd["ranges"], rel_pose=nd["rel_pose"],
                    init_pose=map_local(map_pose, nd["pose"], (0.03, -0.02, 0.01 * (k % 3 - 1))))
               for k, nd in enumerate(nodes[10:])]
    return dict(nodes=nodes[:10], map_pose=map_pose, shape0=shape0, shape=shape, grid=grid,
                alloc=stats["alloc"], queries=queries)


def local_map_steps(oracle, log2_block, seed=3):
    """A local map that starts empty (1 m x 1 m) and takes one scan after the other
    (GridMapBuilder::UpdateGridMap), growing when a scan does not fit. Yields per step the node,
    the shape before and after, the cells, the tracked allocation and a query: the next scan at
    its pose plus an error (None after the last)."""
    case = synth.map_case(seed, n_scans=8, n_beams=720, step=0.4)
    nodes, map_pose = case["nodes"], case["map_pose"]
    shape = initial_shape(0.05, log2_block)
    grid = np.zeros((shape["rows"], shape["cols"]), np.uint16)
    alloc = None
    for k, nd in enumerate(nodes):
        before = shape
        shape, grid, stats = oracle.update_map(shape, grid, map_pose, nd, usable_max=6.0, alloc=alloc)
        alloc = stats["alloc"]
        query = None
        if k + 1 < len(nodes):
            nxt = nodes[k + 1]
            query = dict(geom=geom_of(shape), angles=nxt["angles"], ranges=nxt["ranges"], rel_pose=nxt["rel_pose"],
                         init_pose=map_local(map_pose, nxt["pose"], (0.05, 0.03, -0.01)))
        yield dict(k=k, node=nd, map_pose=map_pose, before=before, shape=shape, grid=grid, alloc=alloc,
                   grew=(stats["row_min"], stats["col_min"]) != (0, 0) or shape != before, query=query)


def sensor_pose(oracle, q):
    return oracle.compound(q["init_pose"], q["rel_pose"])


def divergence(oracle, grid, q, alloc, log2_block):
    """|cost under the tracked allocation - cost under the 16-cell derived bitmap| / cost at the
    query's sensor pose: what the library computed before it carried allocation."""
    p = sensor_pose(oracle, q)
    want = oracle.cost(grid, q["geom"], q["angles"], q["ranges"], p, alloc=alloc, log2_block=log2_block)
    old = oracle.cost(grid, q["geom"], q["angles"], q["ranges"], p, alloc=oracle.derived_alloc(grid, 4),
                      log2_block=4)
    return abs(want - old) / want
