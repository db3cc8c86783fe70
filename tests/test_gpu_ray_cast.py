"""GPU parity of csm_ray_cast with the numpy / Python-integer contract (tests/ray_cast_reference.py): every
named case alone, in both directions; all of them as several sets on several resident maps with shared angle
arrays in one call per parameter set; the same in chunks, with the end points from the host, with a list of
uncertified rays that overflows; maps whose pitch differs from their columns and a map built on the device;
2 000 poses x 90 beams against the host restatement; the cross-check with the ray check; the round trip through the matcher; the map left
untouched; refusals; a map updated between two casts. Records are integers: everything is compared for
equality.

The parameters hold for a whole call, so "all named cases in one call" is one call per parameter set."""
import math

import numpy as np
import pytest

import ray_cast_reference as RC
import ray_check_reference as R
from csm_hip import _lib as L, api, synth

pytestmark = pytest.mark.gpu

CASES = RC.named_cases()
NAMES = [c["name"] for c in CASES]
BASE = 9300                          # 9300 .. 9399: this file's map ids
RANGE = (1.0, 1.0, math.radians(10))


@pytest.fixture(scope="module")
def references():
    return {c["name"]: RC.cast_case(c) for c in CASES}


def _grid_ids():
    """One resident map per distinct grid of the named cases."""
    ids, grids = {}, []
    for c in CASES:
        key = (c["grid"].shape, c["grid"].tobytes())
        if key not in ids:
            ids[key] = BASE + len(grids)
            grids.append(c["grid"])
        c["map_id"] = ids[key]
    return grids


def _upload(ctx):
    grids = _grid_ids()
    assert len(grids) < 60
    for i, g in enumerate(grids):
        ctx.upload_grid(BASE + i, g)
    return len(grids)


def _release(ctx, n):
    for i in range(n):
        if ctx.has_grid(BASE + i):
            ctx.release_grid(BASE + i)


@pytest.fixture(scope="module")
def resident(gpu_ctx):
    n = _upload(gpu_ctx)
    yield gpu_ctx
    _release(gpu_ctx, n)


def _set(c):
    return dict(map_id=c["map_id"], geom=c["geom"], angles=c["angles"], ranges=c["ranges"], poses=c["poses"])


def _groups():
    """The named cases by parameter set, each with one more set that shares the first one's arrays."""
    by = {}
    for c in CASES:
        by.setdefault(tuple(sorted(c["params"].items())), []).append(c)
    return [(dict(key), cs + [cs[0]]) for key, cs in by.items()]


def _run_groups(ctx, references, **extra):
    """Every group through one call; returns the infos after comparing the records."""
    infos = []
    for prm, cs in _groups():
        got, info = ctx.ray_cast([_set(c) for c in cs], **dict(prm, **extra))
        for c, g in zip(cs, got):
            assert np.array_equal(g, references[c["name"]]), c["name"]
        assert info["rays"] == sum(g.size for g in got)
        infos.append(info)
    return infos


@pytest.mark.parametrize("name", NAMES)
def test_named_case_alone(resident, references, name):
    c = CASES[NAMES.index(name)]
    got, info = resident.ray_cast([_set(c)], **c["params"])
    assert got[0].dtype == api.CAST_RECORD and got[0].shape == (c["poses"].shape[0], c["angles"].size)
    assert np.array_equal(got[0], references[name])
    assert info["rays"] == got[0].size and 0 <= info["host_rays"] <= info["rays"]
    assert 0 <= info["cells_to_stop"] <= info["cells_read"]
    if name.startswith("ends_on_cell_edges"):
        assert info["host_rays"] >= 3


def test_sets_on_several_maps_with_shared_angles(resident, references):
    groups = _groups()
    assert max(len({c["map_id"] for c in cs}) for _, cs in groups) >= 4
    assert all(cs[0]["angles"] is cs[-1]["angles"] for _, cs in groups)
    infos = _run_groups(resident, references)
    assert sum(i["host_rays"] for i in infos) > 0           # ends on exact cell edges went through the patch
    assert all(i["device_us"] > 0 for i in infos)


def test_sets_in_chunks(resident, references):
    prm, cs = max(_groups(), key=lambda g: len(g[1]))
    sizes = [48 * c["angles"].size + 64 for c in cs for _ in range(c["poses"].shape[0])]    # scratch_limit_bytes
    assert len(sizes) >= 6
    _run_groups(resident, references, scratch_limit_bytes=max(sizes))
    _run_groups(resident, references, scratch_limit_bytes=1)    # every pose a chunk of its own


@pytest.mark.parametrize("config", [dict(tuning_off=L.TUNE_MAP_HOST_PROJECTION), dict(map_uncertain_cap=1)])
def test_end_points_from_the_host(references, config):
    ctx = api.Context(0, **config)
    try:
        n = _upload(ctx)
        infos = _run_groups(ctx, references)
        if "tuning_off" in config:
            assert all(i["host_rays"] > 0 for i in infos)
        else:
            assert any(i["host_rays"] > 1 for i in infos)   # the list overflowed: the whole chunk from the host
        _release(ctx, n)
    finally:
        ctx.close()


def test_empty_sets_launch_nothing(resident):
    c = CASES[NAMES.index("horizontal")]
    got, info = resident.ray_cast([], **c["params"])
    assert got == [] and info["rays"] == 0
    got, info = resident.ray_cast([dict(_set(c), poses=np.zeros((0, 3))), dict(_set(c), angles=[])], **c["params"])
    assert [g.shape for g in got] == [(0, 2), (1, 0)] and info["rays"] == 0


def test_many_poses_against_the_host_restatement(gpu_ctx):
    case = synth.csm_case(1)
    assert case["grid"].shape == (400, 400)
    mid = BASE + 60
    rng = np.random.RandomState(11)
    res, off_x, off_y = case["geom"]
    n = 2000
    poses = np.stack([off_x + res * rng.uniform(-20, 420, n), off_y + res * rng.uniform(-20, 420, n),
                      rng.uniform(-math.pi, math.pi, n)], axis=1)
    angles = -math.pi + 2 * math.pi * np.arange(90) / 90
    prm = dict(range_max=12.0, range_min=0.1, subpixel_scale=100, unknown_stops=1)
    want = api.host_ray_cast(case["grid"], case["geom"], angles, poses, **prm)
    try:
        gpu_ctx.upload_grid(mid, case["grid"])
        got, info = gpu_ctx.ray_cast([dict(map_id=mid, geom=case["geom"], angles=angles, poses=poses)], **prm)
        assert np.array_equal(got[0], want)
        assert info["rays"] == n * 90 and info["cells_to_stop"] <= info["cells_read"]
        kinds = set(want["kind"].reshape(-1).tolist())
        assert kinds == {RC.NONE, RC.OCCUPIED, RC.UNKNOWN}
    finally:
        if gpu_ctx.has_grid(mid):
            gpu_ctx.release_grid(mid)


def _timeless(summary):
    return {k: v for k, v in summary.items() if not k.endswith("_us")}


@pytest.mark.parametrize("seed", [0, 3])
def test_cross_check_with_the_ray_check(gpu_ctx, seed):
    """The scan's own ranges as limits, end_tolerance 0: on a usable beam whose E is H, the ray check sees a
    blocking cell exactly when the cast stops before E. The map is byte-equal afterwards and a match on it
    returns what it returned before."""
    case = synth.csm_case(seed)
    mid = BASE + 70 + seed
    scan = (case["geom"], case["angles"], case["ranges"], case["rel_pose"])
    scale = 100
    try:
        gpu_ctx.upload_grid(mid, case["grid"])
        before = gpu_ctx.download_level(mid, 0)
        match = gpu_ctx.correlative_match(mid, *scan, case["init_pose"], *RANGE, 4)
        assert match["pose_found"]
        est = tuple(match["estimated_pose"])
        compared = 0
        for robot in (est, (est[0] + 1.0, est[1], est[2])):
            sensor = api.host_compound(robot, case["rel_pose"])
            prm = R.params(usable_range_min=0.0, usable_range_max=6.0, end_tolerance=0)
            q = dict(map_id=mid, geom=case["geom"], angles=case["angles"], ranges=case["ranges"],
                     rel_pose=case["rel_pose"], init_pose=robot)
            _, words = gpu_ctx.ray_check_batch([q], per_beam=True, **prm)
            recs, _ = gpu_ctx.ray_cast([dict(map_id=mid, geom=case["geom"], angles=case["angles"],
                                             ranges=case["ranges"], poses=[sensor])],
                                       range_max=6.0, subpixel_scale=scale, occupied_min=prm["occupied_min"])
            ends = R.beam_ends(case["geom"], case["angles"], case["ranges"], case["rel_pose"], robot, prm)
            for i, w in enumerate(ends):
                if w is None or w["H"] != (w["e"][0] // scale, w["e"][1] // scale):
                    continue
                rec = recs[0][0, i]
                stops_before = rec["kind"] != RC.NONE and (int(rec["cell_x"]), int(rec["cell_y"])) != w["H"]
                assert (int(words[0][i]) > 0) == stops_before, (robot, i)
                compared += 1
        assert compared > 360
        assert np.array_equal(gpu_ctx.download_level(mid, 0), before) and np.array_equal(before, case["grid"])
        again = gpu_ctx.correlative_match(mid, *scan, case["init_pose"], *RANGE, 4)
        assert _timeless(again) == _timeless(match)
    finally:
        if gpu_ctx.has_grid(mid):
            gpu_ctx.release_grid(mid)


def test_round_trip_through_the_matcher(gpu_ctx):
    """A virtual scan from a pose in the room, matched from a guess 7 cm / 0.01 rad off, comes back to the pose
    within one search step on each axis."""
    case = synth.csm_case(2)
    mid = BASE + 80
    res = case["geom"][0]
    pose = tuple(api.host_compound(case["init_pose"], case["rel_pose"]))
    angles = -math.pi + 2 * math.pi * np.arange(360) / 360
    try:
        gpu_ctx.upload_grid(mid, case["grid"])
        a, r = gpu_ctx.virtual_scan(mid, case["geom"], pose, angles, range_max=8.0)
        assert a.size == r.size > 300 and float(r.min()) > 0.0 and float(r.max()) <= 8.0 + res
        guess = (pose[0] + 0.07, pose[1] - 0.07, pose[2] + 0.01)
        out = gpu_ctx.correlative_match(mid, case["geom"], a, r, (0.0, 0.0, 0.0), guess, 0.25, 0.25, math.radians(3), 4)
        assert out["pose_found"]
        step_t = math.acos(1.0 - 0.5 * (res / float(r.max())) ** 2)         # the matcher's angular step
        got = out["estimated_pose"]
        assert abs(got[0] - pose[0]) <= res and abs(got[1] - pose[1]) <= res and abs(got[2] - pose[2]) <= step_t
    finally:
        if gpu_ctx.has_grid(mid):
            gpu_ctx.release_grid(mid)


def test_refusals_leave_the_context_usable(resident, references):
    c = CASES[NAMES.index("horizontal")]
    missing = dict(_set(c), map_id=BASE + 99)
    assert not resident.has_grid(BASE + 99)
    with pytest.raises(api.CsmError) as e:
        resident.ray_cast([_set(c), missing], **c["params"])
    assert e.value.code == L.CSM_ENOENT
    for bad in (dict(range_max=math.inf), dict(range_min=-1.0), dict(occupied_min=0), dict(subpixel_scale=513),
                dict(unknown_stops=2), dict(scratch_limit_bytes=-1)):
        with pytest.raises(api.CsmError) as e:
            resident.ray_cast([_set(c)], **dict(c["params"], **bad))
        assert e.value.code == L.CSM_EINVAL, bad
    with pytest.raises(api.CsmError) as e:
        resident.ray_cast([_set(c), dict(_set(c), poses=[[math.nan, 0.0, 0.0]])], **c["params"])
    assert e.value.code == L.CSM_EINVAL
    got, _ = resident.ray_cast([_set(c)], **c["params"])
    assert np.array_equal(got[0], references["horizontal"])


def test_built_map_with_a_pitch_and_a_map_update(gpu_ctx):
    """A map the device built, cast before and after update_map_with_scan on the same id. (Rows are padded to
    eight cells on the device: among the named cases' grids are widths of 30, 31, 67 and 100 columns, whose
    pitch differs from their columns.)"""
    assert {30, 31, 67, 100} <= {c["grid"].shape[1] for c in CASES}
    case = synth.map_case(2, n_scans=6, n_beams=360)
    mid = BASE + 90
    node = case["nodes"][-1]
    angles = np.asarray(node["angles"], np.float64)[::8]
    try:
        shape, _ = gpu_ctx.construct_map_from_scans(mid, case["shape"], case["map_pose"], case["nodes"][:3])
        local = api.host_inverse_compound(case["map_pose"], node["pose"])
        poses = [api.host_compound(local, node["rel_pose"]), (local[0] + 0.4, local[1] - 0.3, 1.0)]
        seen = []
        for update in (False, True):
            if update:
                for nd in case["nodes"][3:]:
                    shape, _ = gpu_ctx.update_map_with_scan(mid, shape, case["map_pose"], nd)
            grid = gpu_ctx.download_level(mid, 0)
            geom = (shape["res"], shape["off_x"], shape["off_y"])
            prm = dict(range_max=node["max_range"], unknown_stops=1)
            got, _ = gpu_ctx.ray_cast([dict(map_id=mid, geom=geom, angles=angles, poses=poses)], **prm)
            want = api.host_ray_cast(grid, geom, angles, poses, **prm)
            assert np.array_equal(got[0], want)
            assert np.array_equal(want, RC.cast(grid, geom, angles, None, poses, RC.params(
                range_max=node["max_range"], unknown_stops=1, occupied_min=api.host_ray_check_values()[0])))
            seen.append(want)
        assert seen[0].shape != seen[1].shape or not np.array_equal(seen[0], seen[1])   # the update is seen
    finally:
        if gpu_ctx.has_grid(mid):
            gpu_ctx.release_grid(mid)
