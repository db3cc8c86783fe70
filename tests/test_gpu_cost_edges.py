"""CostSquareError and ScanMatcherLinearSolver on the device (csm_cost_covariance_batch,
csm_linear_solver_batch) where test_gpu_cost.py does not look: beams past every edge and corner of
ragged, pitched, non-square maps at other resolutions and offsets; beam counts around the wave and
the workgroup; block allocation given on other block sizes or as missing blocks; the damping and
stop rules of the solver at decisions with a margin; and maps the device built itself, whose
allocation must follow the reference's (Resize / Expand move the blocks, ResetValues keeps them,
updates allocate them). Every case is compared with the oracle (oracle/cost_oracle.cpp) at the
tolerance include/csm_hip.h states."""
import math

import numpy as np
import pytest

from cost_edge_cases import (MARGIN, REL_COST, divergence, fresh_construct, frontend_frames, local_map_steps,
                             margin_ok, sensor_pose)
from csm_hip import synth

pytestmark = pytest.mark.gpu

REL_COV = 1e-8          # covariance entries, relative to the largest entry
ABS_POSE = 1e-7         # refined pose (m, rad) at equal iteration counts
COND_MAX = 1e6          # the covariance is compared where the Hessian is this well conditioned


def _close(a, b, rel):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.all(np.abs(a - b) <= rel * np.maximum(np.abs(b).max(), 1e-300))


def _check_cost(oracle, got, grid, q, pose, alloc, log2_block, where=""):
    """got: one record of cost_covariance_batch at sensor pose `pose`."""
    n = len(q["angles"])
    want = oracle.cost(grid, q["geom"], q["angles"], q["ranges"], pose, alloc=alloc, log2_block=log2_block)
    h, _ = oracle.hessian_residual(grid, q["geom"], q["angles"], q["ranges"], pose, alloc=alloc,
                                   log2_block=log2_block)
    assert abs(got["normalized_cost"] * n - want) <= REL_COST * want, (where, got["normalized_cost"] * n, want)
    assert got["iterations"] == 0 and got["normalized_initial_cost"] == got["normalized_cost"]
    assert _close(got["hessian"], h, REL_COST), (where, got["hessian"], h)
    if np.linalg.cond(h) < COND_MAX:
        cov = oracle.covariance(grid, q["geom"], q["angles"], q["ranges"], pose, 1e4, alloc=alloc,
                                log2_block=log2_block)
        assert _close(got["covariance"], cov, REL_COV), (where, got["covariance"], cov)
    return want


def _check_solver(oracle, got, grid, q, alloc, log2_block, iterations_max=10, threshold=1e-4, lambda_=1e-4,
                  require_margin=True, where=""):
    """got: one record of linear_solver_batch. With every decision of the oracle's run at a margin,
    the device must take them all alike: equal iteration count and damping factor. Returns whether
    the margin held (without require_margin, a run without one is checked on its start only)."""
    w = oracle.linear_solver(grid, q["geom"], q["angles"], q["ranges"], q["rel_pose"], q["init_pose"],
                             iterations_max, threshold, lambda_, 1e4, alloc=alloc, log2_block=log2_block, trace=True)
    assert got["sensor_pose"] == w["sensor_pose"]
    assert abs(got["normalized_initial_cost"] - w["normalized_initial_cost"]) <= \
        REL_COST * w["normalized_initial_cost"], where
    ok = margin_ok(w["trace"], iterations_max, threshold)
    if require_margin:
        assert ok, (where, "no decision margin: choose another case")
    if not ok:
        return False
    assert got["iterations"] == w["iterations"], (where, got["iterations"], w["iterations"])
    assert got["lambda_"] == w["lambda_"], (where, got["lambda_"], w["lambda_"])
    assert np.all(np.abs(np.asarray(got["best_sensor_pose"]) - np.asarray(w["best_sensor_pose"])) <= ABS_POSE), where
    assert np.all(np.abs(np.asarray(got["estimated_pose"]) - np.asarray(w["estimated_pose"])) <= ABS_POSE), where
    assert abs(got["normalized_cost"] - w["normalized_cost"]) <= 1e-9 * w["normalized_cost"], where
    assert _close(got["covariance"], w["covariance"], 1e-6), where
    return True


# ---------------------------------------------------------------- uploaded maps: edges


def _ringed(grid, seed):
    """The room with known cells along the whole map border, so that a read clamped to the first
    or last row / column sees a probability, not the 0.5 of an empty block."""
    g = grid.copy()
    rng = np.random.RandomState(seed)
    for sl in ((slice(0, 2), slice(None)), (slice(-2, None), slice(None)),
               (slice(None), slice(0, 2)), (slice(None), slice(-2, None))):
        g[sl] = rng.randint(20000, 60000, size=g[sl].shape)
    return g


def _reads(geom, shape, pose, angles, ranges):
    """Per beam: which side of the map the hit point lies on and whether a read of the reference's
    GetClosestMapValues (only the upper neighbour clamped) lands inside the map."""
    res, ox, oy = geom
    rows, cols = shape
    a = pose[2] + angles
    fx = (pose[0] + ranges * np.cos(a) - ox) / res
    fy = (pose[1] + ranges * np.sin(a) - oy) / res
    x0, y0 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    xc0, yc0 = np.maximum(x0, 0), np.maximum(y0, 0)
    xc1, yc1 = np.minimum(xc0 + 1, cols - 1), np.minimum(yc0 + 1, rows - 1)
    inside = lambda r, c: (r >= 0) & (r < rows) & (c >= 0) & (c < cols)      # noqa: E731
    reads_in = inside(yc0, xc0) | inside(yc1, xc0) | inside(yc0, xc1) | inside(yc1, xc1)
    return dict(left=x0 < 0, right=x0 >= cols, below=y0 < 0, above=y0 >= rows, reads_in=reads_in)


MAPS = {
    # rows, cols, resolution, offset shift (m): rows / cols off 16, cols off 8 (pitch != cols), non-square
    "ragged_203x317": (203, 317, 0.05, (0.0, 0.0)),
    "tall_333x141_fine": (333, 141, 0.025, (-0.0113, 0.0071)),
    "wide_90x150_coarse": (90, 150, 0.1, (0.0377, -0.0519)),
    "square_128x128": (128, 128, 0.05, (-1.2345, 0.0)),
}


@pytest.mark.parametrize("name", list(MAPS))
def test_beams_past_every_edge_and_corner(gpu_ctx, oracle, name):
    rows, cols, res, shift = MAPS[name]
    grid, geom, segs = synth.make_room(40 + list(MAPS).index(name), rows, cols, res)
    grid = _ringed(grid, rows)
    geom = (geom[0], geom[1] + shift[0], geom[2] + shift[1])
    ext_x, ext_y = cols * res, rows * res
    x0, y0 = geom[1], geom[2]
    reach = 0.8 * max(ext_x, ext_y)
    # sensors inside the map near each edge and corner, and outside it beyond them
    spots = [(fx, fy) for fx in (0.06, 0.5, 0.94) for fy in (0.06, 0.5, 0.94)] + \
            [(-0.1, 0.5), (1.1, 0.5), (0.5, -0.1), (0.5, 1.1), (-0.1, -0.1), (1.1, 1.1), (1.1, -0.1), (-0.1, 1.1)]
    rng = np.random.RandomState(rows + cols)
    queries, poses = [], []
    seen = dict(left=0, right=0, below=0, above=0)
    for i, (fx, fy) in enumerate(spots):
        pose = (x0 + fx * ext_x, y0 + fy * ext_y, 0.3 * i)
        angles = np.linspace(-math.pi, math.pi, 720, endpoint=False)
        ranges = rng.uniform(0.05, reach, angles.size)
        queries.append(dict(map_id=7100, geom=geom, angles=angles, ranges=ranges, rel_pose=(0.0, 0.0, 0.0),
                            init_pose=pose))
        poses.append(pose)
        r = _reads(geom, grid.shape, pose, angles, ranges)
        for side in seen:
            seen[side] += int((r[side] & r["reads_in"]).sum())
    # beams off the map past every edge read cells inside it through the clamp
    assert all(v > 0 for v in seen.values()), seen
    gpu_ctx.upload_grid(7100, grid)
    try:
        got = gpu_ctx.cost_covariance_batch(queries, poses, 1e4)
        alloc = oracle.derived_alloc(grid, 4)
        for i, (q, p, g) in enumerate(zip(queries, poses, got)):
            _check_cost(oracle, g, grid, q, p, alloc, 4, where=(name, i))
        solved = gpu_ctx.linear_solver_batch(queries[:9], 10, 1e-4, 1e-4, 1e4)
        for i, (q, g) in enumerate(zip(queries[:9], solved)):
            _check_solver(oracle, g, grid, q, alloc, 4, require_margin=False, where=(name, i))
    finally:
        gpu_ctx.release_grid(7100)


@pytest.mark.parametrize("corner", ["above_right", "below_left"])
def test_pose_with_every_beam_off_the_map(gpu_ctx, oracle, corner):
    """Every beam far past one corner: the clamped reads land in the corner block, which holds no
    known cell, so every read is 0.5 -- cost exactly 0.25 n, Hessian exactly 0, and a covariance
    that is non-finite where the oracle's is."""
    grid, geom, _ = synth.make_room(7, 203, 317, 0.05)
    assert not grid[:16, :16].any() and not grid[192:, 304:].any()
    ext_x, ext_y = 317 * 0.05, 203 * 0.05
    pose = (geom[1] + ext_x + 3.0, geom[2] + ext_y + 3.0, 0.4) if corner == "above_right" else \
        (geom[1] - 3.0, geom[2] - 3.0, -0.7)
    n = 1081
    angles = np.linspace(-math.pi, math.pi, n, endpoint=False)
    ranges = np.random.RandomState(1).uniform(0.1, 2.5, n)
    r = _reads(geom, grid.shape, pose, angles, ranges)
    assert np.all(r["right"] & r["above"]) if corner == "above_right" else np.all(r["left"] & r["below"])
    q = dict(map_id=7110, geom=geom, angles=angles, ranges=ranges, rel_pose=(0.0, 0.0, 0.0), init_pose=pose)
    gpu_ctx.upload_grid(7110, grid)
    try:
        got = gpu_ctx.cost_covariance_batch([q], [pose], 1e4)[0]
    finally:
        gpu_ctx.release_grid(7110)
    alloc = oracle.derived_alloc(grid, 4)
    want = oracle.cost(grid, geom, angles, ranges, pose, alloc=alloc)
    assert want == 0.25 * n
    assert got["normalized_cost"] * n == 0.25 * n
    h, _ = oracle.hessian_residual(grid, geom, angles, ranges, pose, alloc=alloc)
    assert not h.any() and not np.asarray(got["hessian"]).any()
    cov = oracle.covariance(grid, geom, angles, ranges, pose, 1e4, alloc=alloc)
    assert not np.isfinite(cov).all()
    assert np.array_equal(np.isfinite(got["covariance"]), np.isfinite(cov))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1081, 4096, 5003])
def test_beam_counts_around_wave_and_workgroup(gpu_ctx, oracle, n):
    c = synth.csm_case(3400 + n % 97, rows=203, cols=317, n_beams=n, fov=1.5 * math.pi)
    pose = tuple(np.asarray(c["truth"]) + (0.02, -0.015, 0.01))
    q = dict(map_id=7120, geom=c["geom"], angles=c["angles"], ranges=c["ranges"], rel_pose=c["rel_pose"],
             init_pose=pose)
    gpu_ctx.upload_grid(7120, c["grid"])
    try:
        got = gpu_ctx.cost_covariance_batch([q] * 3, [pose] * 3, 1e4)
        solved = gpu_ctx.linear_solver_batch([q], 10, 1e-4, 1e-4, 1e4)[0]
    finally:
        gpu_ctx.release_grid(7120)
    alloc = oracle.derived_alloc(c["grid"], 4)
    for g in got:
        _check_cost(oracle, g, c["grid"], q, pose, alloc, 4, where=n)
    assert got[0]["normalized_cost"] == got[1]["normalized_cost"] == got[2]["normalized_cost"]
    if n > 1:
        _check_solver(oracle, solved, c["grid"], q, alloc, 4, require_margin=False, where=n)


@pytest.mark.parametrize("log2_block", [0, 2, 3, 5])
def test_block_allocation_on_other_block_sizes(gpu_ctx, oracle, log2_block):
    """csm_set_block_allocation with a bitmap on 2^k-cell blocks (ragged edge blocks included),
    and with None: the rule "allocated iff it holds a known cell" on those blocks (log2 0: every
    cell its own block)."""
    c = synth.csm_case(3500 + log2_block, rows=203, cols=317, n_beams=1080, fov=1.5 * math.pi)
    bs = 1 << log2_block
    dims = (-(-203 // bs), -(-317 // bs))
    rng = np.random.RandomState(log2_block)
    given = (rng.rand(*dims) < 0.7).astype(np.uint8)
    poses = [tuple(np.asarray(c["truth"]) + rng.uniform(-0.05, 0.05, 3) * (1, 1, 0.3)) for _ in range(4)]
    # beams lengthened past the walls end in empty space next to known cells, where the block
    # size decides between 0 and 0.5
    qs = [dict(map_id=7130, geom=c["geom"], angles=c["angles"], ranges=c["ranges"] + extra, rel_pose=c["rel_pose"],
               init_pose=p) for p, extra in zip(poses, (0.0, 0.1, 0.4, 0.8))]
    gpu_ctx.upload_grid(7130, c["grid"])
    try:
        gpu_ctx.set_block_allocation(7130, log2_block, given)
        with_bitmap = gpu_ctx.cost_covariance_batch(qs, poses, 1e4)
        gpu_ctx.set_block_allocation(7130, log2_block, None)
        derived = gpu_ctx.cost_covariance_batch(qs, poses, 1e4)
        solved = gpu_ctx.linear_solver_batch(qs, 10, 1e-4, 1e-4, 1e4)
    finally:
        gpu_ctx.release_grid(7130)
    rule = oracle.derived_alloc(c["grid"], log2_block)
    differ = 0
    for i, (q, p) in enumerate(zip(qs, poses)):
        a = _check_cost(oracle, with_bitmap[i], c["grid"], q, p, given, log2_block, where=("given", i))
        b = _check_cost(oracle, derived[i], c["grid"], q, p, rule, log2_block, where=("derived", i))
        _check_solver(oracle, solved[i], c["grid"], q, rule, log2_block, require_margin=False, where=i)
        differ += abs(b - oracle.cost(c["grid"], q["geom"], q["angles"], q["ranges"], p,
                                      alloc=oracle.derived_alloc(c["grid"], 4))) > MARGIN * b
        assert a != b
    # the block size matters: the 16-cell rule would read these maps differently
    assert differ > 0


@pytest.mark.parametrize("log2_block", [3, 4, 5])
def test_missing_blocks_read_one_half(gpu_ctx, oracle, log2_block):
    """csm_upload_grid_blocks with blocks left out (even ones holding known cells) and all-zero
    blocks kept: a missing block reads 0.5, an allocated unknown cell 0."""
    bs = 1 << log2_block
    br, bc = -(-200 // bs), -(-300 // bs)
    c = synth.csm_case(3600 + log2_block, rows=br * bs, cols=bc * bs, n_beams=1080, fov=1.5 * math.pi)
    grid = c["grid"].copy()
    rng = np.random.RandomState(log2_block)
    mask = (rng.rand(br, bc) < 0.75).astype(np.uint8)
    blocks = []
    for r in range(br):
        for k in range(bc):
            cell = grid[r * bs:(r + 1) * bs, k * bs:(k + 1) * bs]
            if not mask[r, k]:
                cell[:] = 0
            blocks.append(cell.copy() if mask[r, k] else None)
    assert (mask & (oracle.derived_alloc(grid, log2_block) == 0)).any()     # allocated, nothing known
    poses = [tuple(np.asarray(c["truth"]) + rng.uniform(-0.05, 0.05, 3) * (1, 1, 0.3)) for _ in range(4)]
    qs = [dict(map_id=7140, geom=c["geom"], angles=c["angles"], ranges=c["ranges"], rel_pose=c["rel_pose"],
               init_pose=p) for p in poses]
    gpu_ctx.upload_grid_blocks(7140, blocks, br, bc, log2_block)
    try:
        assert np.array_equal(gpu_ctx.download_level(7140, 0), grid)
        got = gpu_ctx.cost_covariance_batch(qs, poses, 1e4)
        solved = gpu_ctx.linear_solver_batch(qs, 10, 1e-4, 1e-4, 1e4)
    finally:
        gpu_ctx.release_grid(7140)
    for i, (q, p) in enumerate(zip(qs, poses)):
        _check_cost(oracle, got[i], grid, q, p, mask, log2_block, where=i)
        _check_solver(oracle, solved[i], grid, q, mask, log2_block, require_margin=False, where=i)


def test_upload_blocks_of_the_wrong_shape_are_refused(gpu_ctx):
    good = np.ones((16, 16), np.uint16)
    for bad in (np.ones((16, 8), np.uint16), np.ones((8, 16), np.uint16), np.ones(256, np.uint16),
                np.ones((32, 32), np.uint16)):
        with pytest.raises(ValueError):
            gpu_ctx.upload_grid_blocks(7150, [good, bad, None, good], 2, 2, 4)
        assert not gpu_ctx.has_grid(7150)


# ---------------------------------------------------------------- the linear solver's rules


def _solver_cases(seeds, err):
    out = []
    for s in seeds:
        c = synth.csm_case(s, n_beams=1080, fov=1.5 * math.pi)
        init = tuple(np.asarray(c["truth"]) + np.asarray(err))
        out.append((c, dict(map_id=7200 + len(out), geom=c["geom"], angles=c["angles"], ranges=c["ranges"],
                            rel_pose=c["rel_pose"], init_pose=init)))
    return out


SOLVER = {
    # name: (iterations_max, threshold, initial lambda, start error)
    "lambda_above_clamp": (10, 1e-4, 1e-3, (0.03, -0.02, 0.01)),
    "lambda_below_clamp": (10, 1e-4, 1e-9, (0.03, -0.02, 0.01)),
    "one_iteration": (1, 1e-4, 1e-4, (0.04, 0.03, -0.01)),
    "threshold_zero": (4, 0.0, 1e-4, (0.04, -0.03, 0.015)),
    "far_start_cost_rises": (10, 1e-4, 1e-4, (0.3, -0.25, 0.05)),
}


@pytest.mark.parametrize("name", list(SOLVER))
def test_linear_solver_decisions(gpu_ctx, oracle, name):
    iterations_max, threshold, lambda_, err = SOLVER[name]
    cases = _solver_cases(range(3700, 3708), err)
    rises = 0
    for c, q in cases:
        w = oracle.linear_solver(c["grid"], q["geom"], q["angles"], q["ranges"], q["rel_pose"], q["init_pose"],
                                 iterations_max, threshold, lambda_, 1e4, alloc=oracle.derived_alloc(c["grid"]),
                                 trace=True)
        rises += any(cost > prev for prev, cost, _ in w["trace"][:-1])
        gpu_ctx.upload_grid(q["map_id"], c["grid"])
    try:
        got = gpu_ctx.linear_solver_batch([q for _, q in cases], iterations_max, threshold, lambda_, 1e4)
    finally:
        for _, q in cases:
            gpu_ctx.release_grid(q["map_id"])
    if name == "far_start_cost_rises":
        assert rises >= 2, rises            # the damping doubles somewhere
    for (c, q), g in zip(cases, got):
        _check_solver(oracle, g, c["grid"], q, oracle.derived_alloc(c["grid"]), 4, iterations_max, threshold,
                      lambda_, where=(name, q["map_id"]))
        if iterations_max == 1:
            assert g["iterations"] == 1
        if threshold == 0.0:
            assert g["iterations"] == iterations_max
        if lambda_ > 1e-4:
            assert g["lambda_"] <= 1e-4 or g["iterations"] == 1


# ---------------------------------------------------------------- maps the device built


def _cost_and_solver(gpu_ctx, oracle, map_id, grid, qs, alloc, log2_block, where):
    qs = [dict(q, map_id=map_id) for q in qs]
    poses = [sensor_pose(oracle, q) for q in qs]
    got = gpu_ctx.cost_covariance_batch(qs, poses, 1e4)
    solved = gpu_ctx.linear_solver_batch(qs, 10, 1e-4, 1e-4, 1e4)
    strict = 0
    for i, q in enumerate(qs):
        _check_cost(oracle, got[i], grid, q, poses[i], alloc, log2_block, where=(where, i))
        strict += _check_solver(oracle, solved[i], grid, q, alloc, log2_block, require_margin=False,
                                where=(where, i))
    return strict


@pytest.mark.parametrize("log2_block", [2, 3, 4, 5])
def test_fresh_construct_on_its_blocks(gpu_ctx, oracle, log2_block):
    """construct_map_from_scans into a fresh id: the map's allocation is on its own blocks
    (PatchSize 2^k); 16-cell blocks are the control where the library's old rule agreed."""
    w = fresh_construct(oracle, log2_block)
    n_div = sum(divergence(oracle, w["grid"], q, w["alloc"], log2_block) > MARGIN for q in w["queries"])
    if log2_block == 4:
        assert np.array_equal(w["alloc"], oracle.derived_alloc(w["grid"], 4))
    else:
        assert n_div >= 2, n_div
    mid = 7300 + log2_block
    shape, _ = gpu_ctx.construct_map_from_scans(mid, w["shape0"], w["map_pose"], w["nodes"])
    try:
        assert shape == w["shape"]
        assert np.array_equal(gpu_ctx.download_level(mid, 0), w["grid"])
        strict = _cost_and_solver(gpu_ctx, oracle, mid, w["grid"], w["queries"], w["alloc"], log2_block,
                                  log2_block)
    finally:
        gpu_ctx.release_grid(mid)
    assert strict >= len(w["queries"]) - 1


@pytest.mark.parametrize("log2_block", [4, 3])
def test_frontend_latest_map_allocation(gpu_ctx, oracle, log2_block):
    """The frontend loop: each frame rebuilds one map id from a sliding window of scans
    (Resize + ResetValues keep the overlapping blocks allocated); the cost at the matched pose and
    the refinement from it read the map as the reference's GridMap does."""
    mid = 7310 + log2_block
    shape_dev = None
    frames = list(frontend_frames(oracle, log2_block))
    n_div = sum(divergence(oracle, f["grid"], f["query"], f["alloc"], log2_block) > MARGIN for f in frames)
    assert n_div >= 5, n_div
    strict = 0
    try:
        for f in frames:
            shape_dev, _ = gpu_ctx.construct_map_from_scans(mid, shape_dev or f["before"], f["map_pose"],
                                                            f["window"])
            assert shape_dev == f["shape"], f["k"]
            strict += _cost_and_solver(gpu_ctx, oracle, mid, f["grid"], [f["query"]], f["alloc"], log2_block,
                                       f["k"])
    finally:
        gpu_ctx.release_grid(mid)
    assert strict >= len(frames) - 5, strict


@pytest.mark.parametrize("log2_block", [4, 3, 5])
def test_local_map_grown_by_updates(gpu_ctx, oracle, log2_block):
    """A local map grown scan by scan with update_map_with_scan, resizes included: allocation is
    the known cells' blocks on the map's own block size (16-cell blocks: the control)."""
    mid = 7320 + log2_block
    steps = list(local_map_steps(oracle, log2_block))
    assert any(s["grew"] for s in steps)
    if log2_block == 4:
        assert all(np.array_equal(s["alloc"], oracle.derived_alloc(s["grid"], 4)) for s in steps)
    else:
        n_div = sum(divergence(oracle, s["grid"], s["query"], s["alloc"], log2_block) > MARGIN
                    for s in steps if s["query"] is not None)
        assert n_div >= 2, n_div
    first = steps[0]["before"]
    gpu_ctx.upload_grid(mid, np.zeros((first["rows"], first["cols"]), np.uint16))
    strict = total = 0
    try:
        for s in steps:
            shape, _ = gpu_ctx.update_map_with_scan(mid, s["before"], s["map_pose"], s["node"],
                                                    usable_range_max=6.0)
            assert shape == s["shape"], s["k"]
            if s["query"] is not None:
                strict += _cost_and_solver(gpu_ctx, oracle, mid, s["grid"], [s["query"]], s["alloc"], log2_block,
                                           s["k"])
                total += 1
    finally:
        gpu_ctx.release_grid(mid)
    assert strict >= 5, (strict, total)     # refinements with every decision at a margin (oracle)
