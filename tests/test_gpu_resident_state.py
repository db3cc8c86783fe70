"""What a context derives from a resident map and keeps between calls, after the map changes
under the same id: box-max levels, the pair-row copies (xg / xgf), the phase-major copies of
the coarse-first search, the pyramid of branch and bound, the block-allocation bitmap and the
recorded HIP graphs. Each cell warms a consumer on a map (three identical calls, so a graph is
recorded), changes the map in place of the same id, calls the consumer twice more and compares
every output with `==` against a fresh map id holding the final cells, uploaded dense, and
against the oracle's matcher where one exists. The final cells themselves are first checked
against the oracle's map (construct_map / update_map).

The block-allocation bitmap follows the reference's GridMap: the cost cells mark every block of
the map allocated (csm_set_block_allocation) before the change. upload_grid starts the map afresh
(a block is allocated iff it holds a known cell); construct_map_from_scans and
update_map_with_scan carry the old bitmap through Resize / Expand, and ResetValues keeps it, so the
blocks of the old map that overlap the new one stay allocated. Their fresh-id reference holds the
final cells plus the oracle's tracked bitmap (construct_map / update_map with alloc=)."""
import itertools
import math

import numpy as np
import pytest

from csm_hip import _lib as L, api, synth

pytestmark = pytest.mark.gpu

MID = 5
CSM = (1.0, 1.0, math.radians(10), 4)
BNB = (2.5, 2.5, 0.5, 2, 0.3, 0.5)
GRID = (0.4, 0.4, 0.2, 0.05, 0.05, 0.025)
_ids = itertools.count(1000)
_WORLDS = {}


# ---------------------------------------------------------------- the map before and after


def _room_queries(segs, geom, seed):
    """Two 1080-beam scans over 1.5 pi (beams share cells: the batch entries take the joint fine
    level with its bound pass, like the loop detectors' scans)."""
    rng = np.random.RandomState(seed)
    qs = []
    for k in range(2):
        truth = (0.3 * (rng.rand() - 0.5), 0.3 * (rng.rand() - 0.5), 0.2 * (rng.rand() - 0.5))
        angles, ranges = synth.cast_scan(segs, truth, 1080, 1.5 * math.pi, 5.7296)
        init = (truth[0] + 0.17, truth[1] - 0.12, truth[2] + 0.02)
        qs.append(dict(geom=geom, angles=angles, ranges=ranges, rel_pose=(0.0, 0.0, 0.0), init_pose=init))
    return qs


def _upload(kind):
    """upload_grid over a map of the same or of another shape; upload_grid_blocks, then upload_grid."""
    a_shape, b_shape = ((300, 300), (300, 300)) if kind != "upload_other_shape" else ((300, 300), (340, 320))
    if kind == "blocks_then_dense":
        a_shape = b_shape = (320, 320)
    seed = {"upload_same_shape": 900, "upload_other_shape": 910, "blocks_then_dense": 920}[kind]
    ga, geom_a, _ = synth.make_room(seed, *a_shape, 0.05)
    gb, geom_b, segs_b = synth.make_room(seed + 1, *b_shape, 0.05)

    def setup(ctx):
        if kind == "blocks_then_dense":
            br, bc = ga.shape[0] // 16, ga.shape[1] // 16
            blocks = [ga[r * 16:(r + 1) * 16, c * 16:(c + 1) * 16] for r in range(br) for c in range(bc)]
            ctx.upload_grid_blocks(MID, [b if b.any() else None for b in blocks], br, bc, 4)
        else:
            ctx.upload_grid(MID, ga)

    def mutate(ctx):
        ctx.upload_grid(MID, gb)

    queries = _room_queries(segs_b, geom_b, seed)
    warm = [dict(q, geom=geom_a) for q in queries]
    return dict(setup=setup, mutate=mutate, grid=gb, queries=queries, warm=warm, cost_alloc=_derived_alloc(gb))


def _map_local(map_pose, pose, err):
    c, s = math.cos(map_pose[2]), math.sin(map_pose[2])
    dx, dy = pose[0] + err[0] - map_pose[0], pose[1] + err[1] - map_pose[1]
    return (c * dx + s * dy, -s * dx + c * dy, pose[2] + err[2] - map_pose[2])


def _pitch_bytes(shape):
    return shape["rows"] * ((shape["cols"] + 7) & ~7) * 2


def _built(kind, oracle):
    """construct_map_from_scans into the old allocation and past it; update_map_with_scan in
    place and with a resize (keep_cells)."""
    case = synth.map_case(930, n_scans=14, n_beams=1080, max_range=5.0, step=0.3)
    nodes, shape0 = case["nodes"], case["shape"]
    map_pose = nodes[0]["pose"]
    near = dict(nodes[0], ranges=np.minimum(nodes[0]["ranges"], 1.5))       # a small first map
    first, second = {"construct_reuse": (nodes[0:8], nodes[2:9]), "construct_grow": ([near], nodes[0:14]),
                     "update_in_place": (nodes[0:10], nodes[5]), "update_grow": (nodes[0:3], nodes[13])}[kind]
    shape1, grid1, _ = oracle.construct_map(shape0, map_pose, first)
    # the cost cells mark every block of the first map allocated before the change
    ones = np.ones((shape1["rows"] >> 4, shape1["cols"] >> 4), np.uint8)
    if kind.startswith("construct"):
        shape2, grid2, st2 = oracle.construct_map(shape1, map_pose, second, alloc=ones)
    else:
        shape2, grid2, st2 = oracle.update_map(shape1, grid1, map_pose, second, alloc=ones)
    if kind == "construct_reuse":
        assert _pitch_bytes(shape2) <= 1.5 * _pitch_bytes(shape1), (shape1, shape2)
    elif kind == "construct_grow":
        assert _pitch_bytes(shape2) > 1.5 * _pitch_bytes(shape1), (shape1, shape2)
    elif kind == "update_in_place":
        assert shape2 == shape1
    else:
        assert (shape2["rows"], shape2["cols"]) != (shape1["rows"], shape1["cols"])

    def setup(ctx):
        got, _ = ctx.construct_map_from_scans(MID, shape0, map_pose, first)
        assert got == shape1

    def mutate(ctx):
        if kind.startswith("construct"):
            got, _ = ctx.construct_map_from_scans(MID, shape1, map_pose, second)
        else:
            got, _ = ctx.update_map_with_scan(MID, shape1, map_pose, second)
        assert got == shape2

    queries, warm = [], []
    for k, err in ((6, (0.04, -0.03, 0.01)), (8, (-0.05, 0.02, -0.015))):
        nd = nodes[k]
        q = dict(angles=nd["angles"], ranges=nd["ranges"], rel_pose=nd["rel_pose"],
                 init_pose=_map_local(map_pose, nd["pose"], err))
        queries.append(dict(q, geom=(shape2["res"], shape2["off_x"], shape2["off_y"])))
        warm.append(dict(q, geom=(shape1["res"], shape1["off_x"], shape1["off_y"])))
    return dict(setup=setup, mutate=mutate, grid=grid2, queries=queries, warm=warm, cost_alloc=st2["alloc"])


MUTATIONS = ["upload_same_shape", "upload_other_shape", "blocks_then_dense", "construct_reuse",
             "construct_grow", "update_in_place", "update_grow"]


def _world(kind, oracle):
    if kind not in _WORLDS:
        _WORLDS[kind] = _upload(kind) if kind.startswith(("upload", "blocks")) else _built(kind, oracle)
    return _WORLDS[kind]


# ---------------------------------------------------------------- consumers


def _with_id(qs, map_id):
    return [dict(q, map_id=map_id) for q in qs]


def _case(grid, q):
    return dict(grid=grid, geom=q["geom"], angles=q["angles"], ranges=q["ranges"], rel_pose=q["rel_pose"],
                init_pose=q["init_pose"])


def _summaries(outs):
    return [(o["pose_found"], o["raw"], o["estimated_pose"]) for o in outs]


def _csm_single(ctx, qs):
    return _summaries([ctx.correlative_match(q["map_id"], q["geom"], q["angles"], q["ranges"], q["rel_pose"],
                                             q["init_pose"], *CSM, 0.0, 0.0) for q in qs])


def _csm_oracle(oracle, grid, qs, got):
    for q, (found, raw, est) in zip(qs, got):
        lit = oracle.csm(_case(grid, q), *CSM)
        assert found == lit["found"], (raw, lit)
        assert (raw["best_x"], raw["best_y"], raw["best_theta"]) == (lit["bestX"], lit["bestY"], lit["bestT"])
        assert raw["score"] == lit["scoreMax"]
        assert est == lit["estimatedPose"]


def _csm_batch(ctx, qs):
    return _summaries(ctx.correlative_match_batch(qs, *CSM, 0.0, 0.0))


def _bnb(ctx, qs):
    return _summaries(ctx.bnb_match_batch(qs, *BNB))


def _bnb_oracle(oracle, grid, qs, got):
    for q, (found, raw, est) in zip(qs, got):
        want = oracle.bnb(_case(grid, q), *BNB)
        assert found == want["found"], (raw, want)
        assert (raw["best_x"], raw["best_y"], raw["best_theta"]) == (want["bestX"], want["bestY"], want["bestT"])
        assert raw["score"] == want["scoreMax"]
        assert est == want["estimatedPose"]


def _grid_search(ctx, qs):
    return [(o["pose_found"], o["candidates"], o["raw"], o["estimated_pose"]) for o in
            (ctx.grid_search_match(q["map_id"], q["geom"], q["angles"], q["ranges"], q["rel_pose"],
                                   q["init_pose"], *GRID) for q in qs)]


def _grid_search_oracle(oracle, grid, qs, got):
    for q, (found, cand, raw, est) in zip(qs, got):
        want = oracle.grid_search(_case(grid, q), *GRID)
        assert cand == want["evaluations"]
        assert found == want["found"]
        assert [raw["best_x"], raw["best_y"], raw["best_theta"]] == want["bestIdx"]
        assert raw["score"] == want["scoreMax"]
        assert est == want["estimatedPose"]


def _poses(qs):
    return np.array([api.host_compound(q["init_pose"], q["rel_pose"]) for q in qs])


def _plain(d):
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def _cost(ctx, qs):
    return ([_plain(o) for o in ctx.cost_covariance_batch(qs, _poses(qs), 1e4)] +
            [_plain(o) for o in ctx.linear_solver_batch(qs, 10, 1e-4, 1e-4, 1e4)])


def _derived_alloc(grid):
    rows, cols = -(-grid.shape[0] // 16) * 16, -(-grid.shape[1] // 16) * 16
    g = np.zeros((rows, cols), grid.dtype)
    g[:grid.shape[0], :grid.shape[1]] = grid
    return (g.reshape(rows // 16, 16, cols // 16, 16).max(axis=(1, 3)) > 0).astype(np.uint8)


def _cost_oracle(oracle, grid, qs, got, alloc):
    for q, p, o in zip(qs, _poses(qs), got[:len(qs)]):
        want = oracle.cost(grid, q["geom"], q["angles"], q["ranges"], p, alloc=alloc)
        assert abs(o["normalized_cost"] * len(q["angles"]) - want) <= 1e-10 * want, (o["normalized_cost"], want)
        cov = np.asarray(oracle.covariance(grid, q["geom"], q["angles"], q["ranges"], p, 1e4, alloc=alloc))
        assert np.all(np.abs(np.asarray(o["covariance"]) - cov) <= 1e-8 * np.abs(cov).max())


def _greedy(ctx, qs):
    return ([_plain(o) for o in ctx.greedy_cost_covariance_batch(qs, _poses(qs))] +
            [_plain(o) for o in ctx.hill_climbing_batch(qs)])


def _greedy_oracle(oracle, grid, qs, got):
    for q, p, o in zip(qs, _poses(qs), got[:len(qs)]):
        cost, cov = api.host_greedy_cost(grid, q["geom"], q["angles"], q["ranges"], p, covariance=True)
        assert o["normalized_cost"] == cost / len(q["angles"])
        assert o["covariance"] == cov.tolist()
    for q, o in zip(qs, got[len(qs):]):
        want = _plain(api.host_hill_climbing(grid, q["geom"], q["angles"], q["ranges"], q["rel_pose"],
                                             q["init_pose"]))
        for key in ("normalized_initial_cost", "normalized_cost", "sensor_pose", "best_sensor_pose",
                    "estimated_pose", "iterations", "refinements", "diff_translation", "diff_rotation",
                    "covariance"):
            assert o[key] == want[key], (key, o[key], want[key])


CONSUMERS = {
    "csm_graphs": (0, _csm_single, _csm_oracle),
    "csm_two_phase": (L.TUNE_FORCE_TWO_PHASE, _csm_single, _csm_oracle),
    "csm_batch": (0, _csm_batch, _csm_oracle),
    "bnb_batch": (0, _bnb, _bnb_oracle),
    "grid_search": (0, _grid_search, _grid_search_oracle),
    "cost_linear": (0, _cost, _cost_oracle),
    "greedy_hill_climbing": (0, _greedy, _greedy_oracle),
}


@pytest.fixture(scope="module")
def refs():
    """Fresh map ids on contexts that never saw the map under test; no graphs on the reference."""
    ctxs = {0: api.Context(0, tuning_off=L.TUNE_NO_GRAPHS),
            L.TUNE_FORCE_TWO_PHASE: api.Context(0, tuning_off=L.TUNE_FORCE_TWO_PHASE | L.TUNE_NO_GRAPHS)}
    yield ctxs
    for c in ctxs.values():
        c.close()


@pytest.mark.parametrize("consumer", list(CONSUMERS))
@pytest.mark.parametrize("mutation", MUTATIONS)
def test_derived_state_follows_the_map(oracle, refs, mutation, consumer):
    tuning, run, check = CONSUMERS[consumer]
    world = _world(mutation, oracle)
    ctx = api.Context(0, tuning_off=tuning)
    try:
        world["setup"](ctx)
        if consumer == "cost_linear":
            rows, cols = ctx.shapes[MID]
            ctx.set_block_allocation(MID, 4, np.ones((-(-rows // 16), -(-cols // 16)), np.uint8))
        warm = _with_id(world["warm"], MID)
        for _ in range(3):
            run(ctx, warm)
        world["mutate"](ctx)
        assert np.array_equal(ctx.download_level(MID, 0), world["grid"])
        qs = _with_id(world["queries"], MID)
        ctx.bound_pass_stats()
        got = [run(ctx, qs) for _ in range(2)]
        if consumer == "csm_two_phase":
            assert ctx.last_search_info()["two_phase"] == 1
        if consumer in ("csm_batch", "bnb_batch"):
            assert sum(ctx.bound_pass_stats()) > 0
    finally:
        ctx.close()
    ref = refs[tuning]
    rid = next(_ids)
    ref.upload_grid(rid, world["grid"])
    try:
        if consumer == "cost_linear":
            ref.set_block_allocation(rid, 4, world["cost_alloc"])
        want = run(ref, _with_id(world["queries"], rid))
    finally:
        ref.release_grid(rid)
    assert got[0] == want
    assert got[1] == want
    if consumer == "cost_linear":
        check(oracle, world["grid"], qs, want, world["cost_alloc"])
    else:
        check(oracle, world["grid"], qs, want)
