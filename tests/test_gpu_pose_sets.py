"""GPU parity of csm_score_pose_sets and csm_pose_set_update with the literal Python of
tests/pose_set_reference.py: records, weights, ancestors and the update record equal the restatement exactly.
The generic cases must stay on the device path (at most 1 % of their poses handed to the host); the forced case
puts a beam exactly on a cell edge and must come back host-projected and still equal."""
import numpy as np
import pytest

import pose_set_reference as R
from csm_hip import _lib as L
from csm_hip import api, synth

pytestmark = pytest.mark.gpu

MAP_ID = 9100


@pytest.fixture(scope="module")
def resident(gpu_ctx):
    grid = R.make_map(1)
    gpu_ctx.upload_grid(MAP_ID, grid)
    yield gpu_ctx, grid
    gpu_ctx.release_grid(MAP_ID)


def _assert_records(rec, grid, geom, angles, ranges, poses, what=None):
    S, K = R.score_poses(grid, geom, angles, ranges, poses)
    got_s, got_k = R.records_sk(rec)
    assert np.array_equal(got_s, S) and np.array_equal(got_k, K), what
    assert not rec["reserved"].any()
    assert set(rec["flags"].tolist()) <= {0, L.POSE_UNCERTAIN | L.POSE_HOST_PROJECTED}
    return S, K


@pytest.mark.parametrize("n_points", R.SWEEP_POINTS)
def test_basic_sweep(resident, n_points):
    ctx, grid = resident
    for n_poses in R.SWEEP_POSES:
        c = R.sweep_case(n_points, n_poses)
        recs, info = ctx.score_pose_sets([dict(map_id=MAP_ID, **c)])
        S, K = _assert_records(recs[0], grid, c["geom"], c["angles"], c["ranges"], c["poses"], (n_points, n_poses))
        assert K.max() > 0
        assert info["poses"] == n_poses and info["uncertain_poses"] <= n_poses // 100, info
        assert info["uncertain_poses"] == int((recs[0]["flags"] != 0).sum())
        assert info["changed_poses"] <= info["uncertain_poses"] and info["device_us"] > 0.0


@pytest.mark.parametrize("n_points, n_poses", [(3, 20001), (5, 33001)])
def test_more_poses_per_workgroup(resident, n_points, n_poses):
    """From 16384 poses a workgroup walks 8, from 32768 on 16 (fewer, larger workgroups); the last one is partial."""
    ctx, grid = resident
    c = R.sweep_case(n_points, n_poses)
    recs, info = ctx.score_pose_sets([dict(map_id=MAP_ID, **c)])
    _assert_records(recs[0], grid, c["geom"], c["angles"], c["ranges"], c["poses"])
    assert info["uncertain_poses"] <= n_poses // 100


def test_poses_outside_and_across_the_borders(resident):
    ctx, grid = resident
    angles, ranges = R.make_scan(11, 65, 0.3, 1.2)
    outside = R.make_poses(11, 70, 0.5, 0.5, centre=(9.0, -7.0))                   # wholly outside: K = 0
    low = R.make_poses(12, 70, 0.3, 0.3, centre=(-1.6, -1.2))                      # negative indices
    high = R.make_poses(13, 70, 0.3, 0.3, centre=(1.6, 1.2))                       # col >= cols, row >= rows
    for name, poses in (("outside", outside), ("low", low), ("high", high)):
        recs, info = ctx.score_pose_sets([dict(map_id=MAP_ID, geom=R.GEOM, angles=angles, ranges=ranges, poses=poses)])
        S, K = _assert_records(recs[0], grid, R.GEOM, angles, ranges, poses, name)
        if name == "outside":
            assert not K.any() and not S.any()
        else:
            assert 0 < K.max() < 65                                                # some beams in, some out
    col, row = api.host_project(R.GEOM, low[0], 0.0, 0, angles, ranges)
    assert col.min() < 0 and row.min() < 0
    col, row = api.host_project(R.GEOM, high[0], 0.0, 0, angles, ranges)
    assert col.max() >= R.COLS and row.max() >= R.ROWS


def test_likelihood_field_as_the_target(resident):
    ctx, grid = resident
    field_id = MAP_ID + 1
    ctx.build_likelihood_map(MAP_ID, field_id, sigma=0.05, resolution=R.GEOM[0])
    try:
        field = ctx.download_level(field_id, 0)
        assert field.shape == grid.shape and not np.array_equal(field, grid)
        c = R.sweep_case(65, 257)
        recs, _ = ctx.score_pose_sets([dict(map_id=field_id, **c)])
        _assert_records(recs[0], field, c["geom"], c["angles"], c["ranges"], c["poses"])
    finally:
        ctx.release_grid(field_id)


def test_map_rebuilt_under_the_same_id_between_calls(gpu_ctx):
    case = synth.map_case(3, n_scans=3, n_beams=360)
    mid = MAP_ID + 2
    node = case["nodes"][1]
    grids = []
    try:
        for nodes in (case["nodes"][:1], case["nodes"]):
            shape, _ = gpu_ctx.construct_map_from_scans(mid, case["shape"], case["map_pose"], nodes)
            geom = (shape["res"], shape["off_x"], shape["off_y"])
            grid = gpu_ctx.download_level(mid, 0)
            grids.append(grid)
            centre = (shape["off_x"] + 0.5 * shape["cols"] * shape["res"],
                      shape["off_y"] + 0.5 * shape["rows"] * shape["res"])
            poses = R.make_poses(21, 65, 1.0, 1.0, centre=centre)
            recs, _ = gpu_ctx.score_pose_sets([dict(map_id=mid, geom=geom, angles=node["angles"],
                                                    ranges=node["ranges"], poses=poses)])
            S, K = _assert_records(recs[0], grid, geom, node["angles"], node["ranges"], poses)
            assert K.max() > 0
        assert grids[0].shape != grids[1].shape or not np.array_equal(grids[0], grids[1])
    finally:
        gpu_ctx.release_grid(mid)


def test_three_sets_two_sharing_a_scan(resident):
    ctx, grid = resident
    other = R.make_map(2, 40, 72)
    other_geom = (0.04, -1.3, -0.9)
    ctx.upload_grid(MAP_ID + 3, other)
    try:
        a65, r65 = R.make_scan(31, 65)
        a360, r360 = R.make_scan(32, 360, 0.2, 1.0)
        sets = [dict(map_id=MAP_ID, geom=R.GEOM, angles=a65, ranges=r65, poses=R.make_poses(31, 130)),
                dict(map_id=MAP_ID + 3, geom=other_geom, angles=a360, ranges=r360, poses=R.make_poses(32, 7)),
                dict(map_id=MAP_ID + 3, geom=other_geom, angles=a65, ranges=r65, poses=R.make_poses(33, 257)),
                dict(map_id=MAP_ID, geom=R.GEOM, angles=a360, ranges=r360, poses=np.zeros((0, 3)))]
        recs, info = ctx.score_pose_sets(sets)
        assert [r.size for r in recs] == [130, 7, 257, 0] and info["poses"] == 394
        for s, rec, g in zip(sets[:3], recs, (grid, other, other)):
            _assert_records(rec, g, s["geom"], s["angles"], s["ranges"], s["poses"])
    finally:
        ctx.release_grid(MAP_ID + 3)


def test_no_set_and_no_pose(resident):
    ctx, _ = resident
    recs, info = ctx.score_pose_sets([])
    assert recs == [] and info["poses"] == 0 and info["uncertain_poses"] == 0
    a, r = R.make_scan(1, 8)
    recs, info = ctx.score_pose_sets([dict(map_id=MAP_ID, geom=R.GEOM, angles=a, ranges=r, poses=np.zeros((0, 3)))])
    assert recs[0].size == 0 and info["poses"] == 0
    out = ctx.pose_set_update(MAP_ID, R.GEOM, a, r, np.zeros((0, 3)), 0.05, n_out=3)
    assert out["ancestors"].tolist() == [-1, -1, -1] and out["update"]["found"] == 0


def test_forced_uncertified_pose(gpu_ctx):
    e = R.edge_case()
    grid = R.make_map(4, known=0.9)
    mid = MAP_ID + 4
    gpu_ctx.upload_grid(mid, grid)
    try:
        recs, info = gpu_ctx.score_pose_sets([dict(map_id=mid, **e)])
        _assert_records(recs[0], grid, e["geom"], e["angles"], e["ranges"], e["poses"])
        assert recs[0]["flags"][0] == L.POSE_UNCERTAIN | L.POSE_HOST_PROJECTED and recs[0]["flags"][1] == 0
        assert info["uncertain_poses"] >= 1 and info["host_us"] > 0.0
        out = gpu_ctx.pose_set_update(mid, e["geom"], e["angles"], e["ranges"], e["poses"], 0.05, n_out=5, offset=3)
        S, K = R.score_poses(grid, e["geom"], e["angles"], e["ranges"], e["poses"])
        w, a, upd = R.update(S.tolist(), K.tolist(), 4, 0.05, 0.0, 5, 3)
        assert out["weights"].tolist() == w and out["ancestors"].tolist() == a and out["update"] == upd
        assert out["records"]["flags"][0] & L.POSE_HOST_PROJECTED
    finally:
        gpu_ctx.release_grid(mid)


@pytest.mark.parametrize("n_points, n_poses, temperature, threshold, n_out, offset", [
    (360, 1000, 0.05, 0.1, None, 0),
    (360, 1000, 2e-4, 0.1, 7, (1 << 64) - 1),             # most weights 0
    (65, 257, 0.02, 0.0, 4 * 257, 0x123456789ABCDEF),
    (64, 1025, 0.3, 0.3, 1, 77),                          # two tiles of k_pose_weights, one output
    (63, 1, 0.05, 0.0, 9, 5),                             # one pose
    (360, 300, 0.05, 0.99, 50, 1),                        # none eligible (K >= 357 of about 0.6 * 360)
    (1, 64, 0.05, 0.0, 64, 0),                            # one beam: few distinct keys, ties
    (1100, 70, 0.05, 0.1, None, 9),                       # more beams than one LDS tile of k_pose_score
])
def test_update_equals_the_restatement(resident, n_points, n_poses, temperature, threshold, n_out, offset):
    ctx, grid = resident
    c = R.sweep_case(n_points, n_poses)
    out = ctx.pose_set_update(MAP_ID, c["geom"], c["angles"], c["ranges"], c["poses"], temperature, threshold,
                              n_out, offset)
    S, K = _assert_records(out["records"], grid, c["geom"], c["angles"], c["ranges"], c["poses"])
    w, a, upd = R.update(S.tolist(), K.tolist(), n_points, temperature, threshold, n_out, offset)
    assert out["weights"].tolist() == w
    assert out["ancestors"].tolist() == a
    assert out["update"] == upd
    assert out["info"]["uncertain_poses"] <= n_poses // 100
    host = api.host_pose_set_update(out["records"], n_points, temperature, threshold, n_out, offset)
    assert host[0].tolist() == w and host[1].tolist() == a and host[2] == upd
    if threshold == 0.99:
        assert upd["found"] == 0 and set(a) == {-1}


def test_refusals_run_nothing(resident):
    ctx, _ = resident
    a, r = R.make_scan(1, 8)
    poses = R.make_poses(1, 4)
    good = dict(map_id=MAP_ID, geom=R.GEOM, angles=a, ranges=r, poses=poses)
    bad_pose = poses.copy()
    bad_pose[2, 1] = np.inf
    bad_angle = a.copy()
    bad_angle[0] = np.nan
    far = poses.copy()
    far[0, 0] = 0.05 * 2.0 ** 30
    for bad in (dict(good, poses=bad_pose), dict(good, angles=bad_angle),
                dict(good, poses=far), dict(good, angles=a[:0], ranges=r[:0])):
        with pytest.raises(api.CsmError) as e:
            ctx.score_pose_sets([good, bad])
        assert e.value.code == L.CSM_EINVAL
    assert not ctx.has_grid(MAP_ID + 77)
    with pytest.raises(api.CsmError) as e:                                          # a map that is not resident
        ctx.score_pose_sets([good, dict(good, map_id=MAP_ID + 77)])
    assert e.value.code == L.CSM_ENOENT
    with pytest.raises(api.CsmError) as e:
        ctx.pose_set_update(MAP_ID + 77, R.GEOM, a, r, poses, 0.05)
    assert e.value.code == L.CSM_ENOENT
    for kw in (dict(n_out=-1), dict(n_out=(1 << 18) + 1), dict(temperature=0.0), dict(temperature=float("nan"))):
        args = dict(temperature=0.05, n_out=4)
        args.update(kw)
        with pytest.raises(api.CsmError) as e:
            ctx.pose_set_update(MAP_ID, R.GEOM, a, r, poses, **args)
        assert e.value.code == L.CSM_EINVAL
    recs, _ = ctx.score_pose_sets([good])                                           # the context is still good
    assert recs[0].size == 4


def test_destroy_returns_every_byte():
    before = api.debug_live_bytes()
    ctx = api.Context(0)
    grid = R.make_map(1)
    ctx.upload_grid(5, grid)
    c = R.sweep_case(65, 257)
    ctx.pose_set_update(5, c["geom"], c["angles"], c["ranges"], c["poses"], 0.05)
    e = R.edge_case()
    ctx.score_pose_sets([dict(map_id=5, **e)])                                      # the rescore's buffers too
    assert api.debug_live_bytes() != before
    ctx.close()
    assert api.debug_live_bytes() == before
