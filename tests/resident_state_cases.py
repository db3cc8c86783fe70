"""The worlds of tests/test_gpu_resident_state.py: a map before and after a change under the same id, the
queries asked of it, and the numpy references of the consumers that read it. No GPU is touched here:
tests/test_cpu_resident_state_cases.py imports the worlds and proves that every cell means something (stale
state would change its answer), tests/test_gpu_resident_state.py runs them.

A world is a dict: setup(ctx) puts the first map under MID, mutate(ctx) changes it, `before` / `grid` are the
cells before and after, `warm` / `queries` two queries in the geometry before and after, `cost_alloc` the
block-allocation bitmap the reference keeps for the final map, `qid` the id the consumers query after the
change (MID, except where the change moves the map to another id) and `gone` an id that must then be refused.

The seven first worlds carry 1080-beam scans, as the batch matchers need them (beams share cells). The five
new worlds are built on the same rooms and trajectories, and the consumers added with them (peaks, covariance,
prior, pose sets, ray check) run on the same two queries: their numpy references take about a second per
world at 1080 beams, so no second set of 360-beam queries was needed."""
import math

import numpy as np

import global_map_cases as GM
import likelihood_reference as LR
import peaks_reference as PR
import pose_set_reference as PS
import prior_reference as P
import ray_check_reference as RC
import volume_reference as VR
from csm_hip import synth
from oracle import oracle as O

MID = 5
OTHER = MID + 2                      # the second map of the batch builder's call
SRC = MID + 3                        # the occupancy map a likelihood field under MID is built from
CSM = (1.0, 1.0, math.radians(10), 4)
BNB = (2.5, 2.5, 0.5, 2, 0.3, 0.5)
GRID = (0.4, 0.4, 0.2, 0.05, 0.05, 0.025)
RANGE, LOW = CSM[:3], CSM[3]
K_MAX, EXCL = 4, (3, 3, 2)
TAU = 0.02
# score units per m^2 / rad^2: strong enough to pull the winner off the plain arg-max towards the initial
# pose, 0.17 m / 0.12 m / 0.02 rad away (proven for every query in tests/test_cpu_resident_state_cases.py)
LAMBDA = np.array([[30.0, 5.0, 8.0], [5.0, 20.0, -6.0], [8.0, -6.0, 400.0]])
N_POSES = 257
GLOBAL_RANK = (2, 4)                 # rank_direct_max, rank_tile of the global_parts world
_WORLDS = {}
_REFS = {}


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


def _derived_alloc(grid):
    rows, cols = -(-grid.shape[0] // 16) * 16, -(-grid.shape[1] // 16) * 16
    g = np.zeros((rows, cols), grid.dtype)
    g[:grid.shape[0], :grid.shape[1]] = grid
    return (g.reshape(rows // 16, 16, cols // 16, 16).max(axis=(1, 3)) > 0).astype(np.uint8)


def _upload(kind):
    """upload_grid over a map of the same or of another shape; upload_grid_blocks, then upload_grid;
    release_grid, then upload_grid under the same id or under the next one."""
    a_shape, b_shape = ((300, 300), (300, 300)) if kind != "upload_other_shape" else ((300, 300), (340, 320))
    if kind == "blocks_then_dense":
        a_shape = b_shape = (320, 320)
    seed = {"upload_same_shape": 900, "upload_other_shape": 910, "blocks_then_dense": 920,
            "release_reupload": 940, "release_other_id": 950}[kind]
    ga, geom_a, _ = synth.make_room(seed, *a_shape, 0.05)
    gb, geom_b, segs_b = synth.make_room(seed + 1, *b_shape, 0.05)
    qid = MID + 1 if kind == "release_other_id" else MID

    def setup(ctx):
        if kind == "blocks_then_dense":
            br, bc = ga.shape[0] // 16, ga.shape[1] // 16
            blocks = [ga[r * 16:(r + 1) * 16, c * 16:(c + 1) * 16] for r in range(br) for c in range(bc)]
            ctx.upload_grid_blocks(MID, [b if b.any() else None for b in blocks], br, bc, 4)
        else:
            ctx.upload_grid(MID, ga)

    def mutate(ctx):
        if kind.startswith("release"):
            ctx.release_grid(MID)
        ctx.upload_grid(qid, gb)

    queries = _room_queries(segs_b, geom_b, seed)
    warm = [dict(q, geom=geom_a) for q in queries]
    return dict(setup=setup, mutate=mutate, before=ga, grid=gb, queries=queries, warm=warm,
                queries_new=queries, warm_new=warm,       # the room scans serve old and new consumers alike
                cost_alloc=_derived_alloc(gb), qid=qid, gone=MID if qid != MID else None)


def _map_local(map_pose, pose, err):
    c, s = math.cos(map_pose[2]), math.sin(map_pose[2])
    dx, dy = pose[0] + err[0] - map_pose[0], pose[1] + err[1] - map_pose[1]
    return (c * dx + s * dy, -s * dx + c * dy, pose[2] + err[2] - map_pose[2])


def _pitch_bytes(shape):
    return shape["rows"] * ((shape["cols"] + 7) & ~7) * 2


def _geom(shape):
    return (shape["res"], shape["off_x"], shape["off_y"])


def _trajectory():
    case = synth.map_case(930, n_scans=14, n_beams=1080, max_range=5.0, step=0.3)
    return case["nodes"], case["shape"], case["nodes"][0]["pose"]


OLD_PICKS = ((6, (0.04, -0.03, 0.01)), (8, (-0.05, 0.02, -0.015)))
# the last scan of the trajectory from two poses three cells off: its windows stay clear of the final map's
# low edge band in every built world, and the arg-max is far enough from the centre for a prior to move it
NEW_PICKS = ((13, (0.17, -0.12, 0.02)), (13, (-0.13, 0.16, -0.03)))


def _node_queries(nodes, map_pose, geom_before, geom_after, picks=OLD_PICKS):
    queries, warm = [], []
    for k, err in picks:
        nd = nodes[k]
        q = dict(angles=nd["angles"], ranges=nd["ranges"], rel_pose=nd["rel_pose"],
                 init_pose=_map_local(map_pose, nd["pose"], err))
        queries.append(dict(q, geom=geom_after))
        warm.append(dict(q, geom=geom_before))
    return queries, warm


def _built(kind, oracle):
    """construct_map_from_scans into the old allocation and past it; update_map_with_scan in
    place and with a resize (keep_cells)."""
    nodes, shape0, map_pose = _trajectory()
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

    queries, warm = _node_queries(nodes, map_pose, _geom(shape1), _geom(shape2))
    queries_new, warm_new = _node_queries(nodes, map_pose, _geom(shape1), _geom(shape2), NEW_PICKS)
    return dict(setup=setup, mutate=mutate, before=grid1, grid=grid2, queries=queries, warm=warm,
                queries_new=queries_new, warm_new=warm_new,
                cost_alloc=st2["alloc"], qid=MID, gone=None)


def _batch_build(oracle):
    """construct_maps_from_scans: MID rebuilt next to a second, smaller map under OTHER, in one call. The
    order of the two jobs is the caller's (mutate(ctx, reverse)): the result must not depend on it."""
    nodes, shape0, map_pose = _trajectory()
    first, second = nodes[1:7], nodes[4:13]
    small = [dict(nd, ranges=np.minimum(nd["ranges"], 2.0)) for nd in nodes[0:3]]
    shape1, grid1, _ = oracle.construct_map(shape0, map_pose, first)
    ones = np.ones((shape1["rows"] >> 4, shape1["cols"] >> 4), np.uint8)
    shape2, grid2, st2 = oracle.construct_map(shape1, map_pose, second, alloc=ones)
    shape_o, grid_o, _ = oracle.construct_map(shape0, map_pose, small)
    assert grid_o.shape != grid2.shape

    def setup(ctx):
        got, _ = ctx.construct_map_from_scans(MID, shape0, map_pose, first)
        assert got == shape1

    def mutate(ctx, reverse=False):
        jobs = [dict(map_id=MID, shape=shape1, map_pose=map_pose, nodes=second),
                dict(map_id=OTHER, shape=shape0, map_pose=map_pose, nodes=small)]
        results, binfo = ctx.construct_maps_from_scans(jobs[::-1] if reverse else jobs)
        got = dict(zip((OTHER, MID) if reverse else (MID, OTHER), results))
        assert got[MID][2] == 0 and got[OTHER][2] == 0 and binfo["chunks"] == 1
        assert got[MID][0] == shape2 and got[OTHER][0] == shape_o
        assert np.array_equal(ctx.download_level(OTHER, 0), grid_o)

    queries, warm = _node_queries(nodes, map_pose, _geom(shape1), _geom(shape2))
    queries_new, warm_new = _node_queries(nodes, map_pose, _geom(shape1), _geom(shape2), NEW_PICKS)
    return dict(setup=setup, mutate=mutate, before=grid1, grid=grid2, queries=queries, warm=warm,
                queries_new=queries_new, warm_new=warm_new,
                cost_alloc=st2["alloc"], qid=MID, gone=None)


def _global_parts(oracle):
    """construct_global_map on MID, one node per part, with rank settings under which every part ranks
    cells by counting, by sorting and by tiles (`job` / `shape` are there for the CPU proof of that)."""
    nodes, shape0, map_pose = _trajectory()
    first, second = nodes[0:6], nodes[3:11]
    shape1, grid1, _ = oracle.construct_map(shape0, map_pose, first)
    ones = np.ones((shape1["rows"] >> 4, shape1["cols"] >> 4), np.uint8)
    shape2, grid2, st2 = oracle.construct_map(shape1, map_pose, second, alloc=ones)

    def setup(ctx):
        got, _ = ctx.construct_map_from_scans(MID, shape0, map_pose, first)
        assert got == shape1

    def mutate(ctx):
        got, _, ginfo = ctx.construct_global_map(MID, shape1, map_pose, second, scratch_limit_bytes=1,
                                                 rank_direct_max=GLOBAL_RANK[0], rank_tile=GLOBAL_RANK[1])
        assert got == shape2
        assert ginfo["parts"] == len(second), ginfo
        for path in GM.ALL:
            assert ginfo[path + "_cells"] > 0, (path, ginfo)

    queries, warm = _node_queries(nodes, map_pose, _geom(shape1), _geom(shape2))
    queries_new, warm_new = _node_queries(nodes, map_pose, _geom(shape1), _geom(shape2), NEW_PICKS)
    return dict(setup=setup, mutate=mutate, before=grid1, grid=grid2, queries=queries, warm=warm,
                queries_new=queries_new, warm_new=warm_new,
                cost_alloc=st2["alloc"], qid=MID, gone=None,
                job=dict(nodes=second, map_pose=map_pose), shape=shape2)


FIELD_SIGMAS = (0.05, 0.1)


def _field(grid, sigma, res):
    R = LR.radius(sigma, res)
    return LR.likelihood_map(grid, LR.kernel(sigma, res, R), R)


def _field_rebuild(oracle):
    """MID is the likelihood field of the occupancy map under SRC. The source takes one more scan in place,
    then the field is rebuilt into MID with another sigma (take_grid: levels, copies and bitmap start anew)."""
    nodes, shape0, map_pose = _trajectory()
    shape1, grid1, _ = oracle.construct_map(shape0, map_pose, nodes[0:10])
    shape2, grid2, _ = oracle.update_map(shape1, grid1, map_pose, nodes[5])
    assert shape2 == shape1
    res = shape1["res"]
    before, after = _field(grid1, FIELD_SIGMAS[0], res), _field(grid2, FIELD_SIGMAS[1], res)

    def setup(ctx):
        got, _ = ctx.construct_map_from_scans(SRC, shape0, map_pose, nodes[0:10])
        assert got == shape1
        ctx.build_likelihood_map(SRC, MID, FIELD_SIGMAS[0], res)

    def mutate(ctx):
        got, _ = ctx.update_map_with_scan(SRC, shape1, map_pose, nodes[5])
        assert got == shape2
        assert np.array_equal(ctx.download_level(SRC, 0), grid2)        # the downloaded source is the oracle's
        ctx.build_likelihood_map(SRC, MID, FIELD_SIGMAS[1], res)

    queries, warm = _node_queries(nodes, map_pose, _geom(shape1), _geom(shape2))
    queries_new, warm_new = _node_queries(nodes, map_pose, _geom(shape1), _geom(shape2), NEW_PICKS)
    return dict(setup=setup, mutate=mutate, before=before, grid=after, queries=queries, warm=warm,
                queries_new=queries_new, warm_new=warm_new,
                cost_alloc=_derived_alloc(after), qid=MID, gone=None, derived_alloc_only=True)


OLD_MUTATIONS = ["upload_same_shape", "upload_other_shape", "blocks_then_dense", "construct_reuse",
                 "construct_grow", "update_in_place", "update_grow"]
NEW_MUTATIONS = ["batch_build", "global_parts", "field_rebuild", "release_reupload", "release_other_id"]
MUTATIONS = OLD_MUTATIONS + NEW_MUTATIONS
# the three ways level 0 changes while the id and the DeviceGrid stay or are replaced under the same id
LEVEL_MUTATIONS = ["update_in_place", "global_parts", "field_rebuild"]


def world(kind, oracle=O):
    if kind not in _WORLDS:
        if kind.startswith(("upload", "blocks", "release")):
            w = _upload(kind)
        elif kind in ("batch_build", "global_parts", "field_rebuild"):
            w = dict(batch_build=_batch_build, global_parts=_global_parts, field_rebuild=_field_rebuild)[kind](oracle)
        else:
            w = _built(kind, oracle)
        for g in (w["before"], w["grid"]):
            g.setflags(write=False)
        _WORLDS[kind] = w
    return _WORLDS[kind]


# ---------------------------------------------------------------- numpy references of the new consumers


def case_of(grid, q):
    return dict(grid=grid, geom=q["geom"], angles=q["angles"], ranges=q["ranges"], rel_pose=q["rel_pose"],
                init_pose=q["init_pose"])


def pose_set(q, k):
    """257 sensor poses around the query's initial sensor pose (0.3 m, 0.2 rad each way)."""
    s = O.compound(q["init_pose"], q["rel_pose"])
    rng = np.random.RandomState(7000 + k)
    return np.stack([s[0] + rng.uniform(-0.3, 0.3, N_POSES), s[1] + rng.uniform(-0.3, 0.3, N_POSES),
                     s[2] + rng.uniform(-0.2, 0.2, N_POSES)], axis=1)


# the scans' longest beams (5.0 m and 5.7296 m: no return) are not walked
RAY = RC.params(usable_range_max=5.0)


def reference_of(consumer, grid, qs):
    """The numpy reference of a new consumer on `grid` for the queries `qs` (uncached)."""
    out = []
    for k, q in enumerate(qs):
        case = case_of(grid, q)
        if consumer == "peaks":
            rec, cf, win = PR.peaks(case, *RANGE, LOW, K_MAX, EXCL)
            out.append(dict(records=rec, win=win, band=cf["touchesBand"]))
        elif consumer == "volume_cov":
            ref, win = VR.summary(case, *RANGE, LOW, TAU)
            out.append(dict(summary=ref, win=win))
        elif consumer == "prior":
            vol = P.volume(case, *RANGE, LOW)
            out.append(dict(prior=P.prior(vol, case, LAMBDA)[0], win=vol["win"], band=vol["cf"]["touchesBand"]))
        elif consumer == "pose_sets":
            S, K = PS.score_poses(grid, q["geom"], q["angles"], q["ranges"], pose_set(q, k))
            out.append(dict(S=S.tolist(), K=K.tolist()))
        elif consumer == "ray_check":
            rec, words = RC.ray_check(grid, q["geom"], q["angles"], q["ranges"], q["rel_pose"], q["init_pose"],
                                      RAY)
            out.append(dict(record=rec, words=words.tolist()))
        else:
            raise KeyError(consumer)
    return out


def reference(kind, consumer, when="after"):
    """reference_of on a world's final map with its queries (when = "after") or on its first map with the
    warm queries ("before"): computed once, shared, never changed."""
    key = (kind, consumer, when)
    if key not in _REFS:
        w = world(kind)
        _REFS[key] = reference_of(consumer, *((w["grid"], w["queries_new"]) if when == "after" else
                                              (w["before"], w["warm_new"])))
    return _REFS[key]


def boxmax_in_window(grid, q, low=LOW):
    """The box-max(low) cells a search of q's window reads: the level cropped to the hull of the hit cells of
    every slice, widened by the window (clipped to the map)."""
    (wx, wy, wt), _, _, col, row = PR.window_of(case_of(grid, q), *RANGE)
    level = O.boxmax(grid, low)
    r0, r1 = max(int(row.min()) - wy, 0), min(int(row.max()) + wy + low, grid.shape[0])
    c0, c1 = max(int(col.min()) - wx, 0), min(int(col.max()) + wx + low, grid.shape[1])
    return level[r0:r1, c0:c1]
