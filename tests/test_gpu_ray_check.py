"""GPU parity of csm_ray_check_batch with the numpy definition (tests/ray_check_reference.py): every named
case alone, the named cases batched on several resident maps with shared scan arrays, in chunks, with the hit
points from the host, without per-beam words; two 400 x 400 cases at the matcher's pose and 1 m off; the map
left untouched; a map that is not resident; a map updated between two checks. Everything is an integer:
records (host_beams aside) and per-beam words are compared for equality.

The parameters hold for a whole call, so "all named cases in one call" is one call per parameter set: the
default set holds most cases, on several maps; each sweep set holds its case."""
import math

import numpy as np
import pytest

import ray_check_reference as R
from csm_hip import _lib as L, api, synth

pytestmark = pytest.mark.gpu

CASES = R.named_cases()
NAMES = [c["name"] for c in CASES]
BASE = 8500                          # 8500 .. 8599: this file's map ids
RANGE = (1.0, 1.0, math.radians(10))


@pytest.fixture(scope="module")
def references():
    return {c["name"]: R.check_case(c) for c in CASES}


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
    for i, g in enumerate(_grid_ids()):
        ctx.upload_grid(BASE + i, g)
    return len(_grid_ids())


def _release(ctx, n):
    for i in range(n):
        if ctx.has_grid(BASE + i):
            ctx.release_grid(BASE + i)


@pytest.fixture(scope="module")
def resident(gpu_ctx):
    n = _upload(gpu_ctx)
    yield gpu_ctx
    _release(gpu_ctx, n)


def _query(c):
    return dict(map_id=c["map_id"], geom=c["geom"], angles=c["angles"], ranges=c["ranges"], rel_pose=c["rel_pose"],
                init_pose=c["pose"])


def _groups():
    """The named cases by parameter set, each with one more query that shares the first one's scan arrays."""
    by = {}
    for c in CASES:
        by.setdefault(tuple(sorted(c["params"].items())), []).append(c)
    return [(dict(key), cs + [cs[0]]) for key, cs in by.items()]


def _run_groups(ctx, references, **extra):
    """Every group through one call; returns the records in call order after comparing them."""
    records = []
    for prm, cs in _groups():
        got, words = ctx.ray_check_batch([_query(c) for c in cs], per_beam=True, **dict(prm, **extra))
        for c, g, w in zip(cs, got, words):
            want, want_words = references[c["name"]]
            assert R.strip(g) == want, c["name"]
            assert np.array_equal(w, want_words), c["name"]
        records += got
    return records


@pytest.mark.parametrize("name", NAMES)
def test_named_case_alone(resident, references, name):
    c = CASES[NAMES.index(name)]
    want, want_words = references[name]
    got, words = resident.ray_check_batch([_query(c)], per_beam=True, **c["params"])
    assert R.strip(got[0]) == want
    assert np.array_equal(words[0], want_words)
    assert 0 <= got[0]["host_beams"] <= got[0]["usable"]


def test_batches_on_several_maps_with_shared_scans(resident, references):
    groups = _groups()
    assert max(len({c["map_id"] for c in cs}) for _, cs in groups) >= 4
    assert all(cs[0]["angles"] is cs[-1]["angles"] for _, cs in groups)
    records = _run_groups(resident, references)
    assert all(0 <= r["host_beams"] <= r["usable"] for r in records)
    assert sum(r["host_beams"] for r in records) > 0        # beams on exact cell edges went through the patch


def test_batches_in_chunks(resident, references):
    prm, cs = max(_groups(), key=lambda g: len(g[1]))
    sizes = [36 * c["angles"].size + 256 for c in cs]       # csm_ray_check_params.scratch_limit_bytes
    limit = max(sizes)
    chunks, held = 1, 0
    for s in sizes:
        if held and held + s > limit:
            chunks, held = chunks + 1, 0
        held += s
    assert chunks >= 3
    _run_groups(resident, references, scratch_limit_bytes=limit)
    _run_groups(resident, references, scratch_limit_bytes=1)   # every query a chunk of its own


@pytest.mark.parametrize("config", [dict(tuning_off=L.TUNE_MAP_HOST_PROJECTION), dict(map_uncertain_cap=1)])
def test_hit_points_from_the_host(references, config):
    ctx = api.Context(0, **config)
    try:
        n = _upload(ctx)
        records = _run_groups(ctx, references)
        if "tuning_off" in config:
            assert all(r["host_beams"] == r["usable"] for r in records)
        else:
            assert any(r["host_beams"] == r["usable"] > 1 for r in records)    # the list overflowed
        _release(ctx, n)
    finally:
        ctx.close()


def test_without_per_beam_words(resident, references):
    for prm, cs in _groups():
        got = resident.ray_check_batch([_query(c) for c in cs], **prm)
        assert [R.strip(g) for g in got] == [references[c["name"]][0] for c in cs]


def _timeless(summary):
    return {k: v for k, v in summary.items() if not k.endswith("_us")}


@pytest.mark.parametrize("seed", [0, 3])
def test_matcher_pose_and_a_pose_one_metre_off(gpu_ctx, seed):
    case = synth.csm_case(seed)
    assert case["grid"].shape == (400, 400) and case["angles"].size == 360
    mid = BASE + 50 + seed
    scan = (case["geom"], case["angles"], case["ranges"], case["rel_pose"])
    try:
        gpu_ctx.upload_grid(mid, case["grid"])
        before = gpu_ctx.download_level(mid, 0)
        match = gpu_ctx.correlative_match(mid, *scan, case["init_pose"], *RANGE, 4)
        assert match["pose_found"]
        est = tuple(match["estimated_pose"])
        off = (est[0] + 1.0, est[1], est[2])
        q = dict(map_id=mid, geom=case["geom"], angles=case["angles"], ranges=case["ranges"],
                 rel_pose=case["rel_pose"], init_pose=case["init_pose"])
        prm = R.params(usable_range_max=6.0)
        got, words = gpu_ctx.ray_check_batch([q, q], poses=[est, off], per_beam=True, **prm)
        for pose, g, w in zip((est, off), got, words):
            want, want_words = R.ray_check(case["grid"], *scan, pose, prm)
            assert R.strip(g) == want
            assert np.array_equal(w, want_words)
            assert g["host_beams"] <= g["usable"]
        # the map is untouched: its cells, and what a search on it returns
        assert np.array_equal(gpu_ctx.download_level(mid, 0), before) and np.array_equal(before, case["grid"])
        again = gpu_ctx.correlative_match(mid, *scan, case["init_pose"], *RANGE, 4)
        assert _timeless(again) == _timeless(match)
    finally:
        if gpu_ctx.has_grid(mid):
            gpu_ctx.release_grid(mid)


def test_a_map_that_is_not_resident(resident, references):
    c = CASES[NAMES.index("horizontal")]
    missing = dict(_query(c), map_id=BASE + 99)
    assert not resident.has_grid(BASE + 99)
    with pytest.raises(api.CsmError) as e:
        resident.ray_check_batch([_query(c), missing], **c["params"])
    assert e.value.code == L.CSM_ENOENT
    with pytest.raises(api.CsmError) as e:
        resident.ray_check_batch([_query(c)], **dict(c["params"], free_max=c["params"]["occupied_min"]))
    assert e.value.code == L.CSM_EINVAL
    got = resident.ray_check_batch([_query(c)], **c["params"])
    assert R.strip(got[0]) == references["horizontal"][0]


def test_check_sees_a_map_update(gpu_ctx):
    case = synth.map_case(2, n_scans=6, n_beams=360)
    mid = BASE + 60
    node = case["nodes"][-1]
    prm = R.params(usable_range_min=node["min_range"], usable_range_max=node["max_range"])
    try:
        shape, _ = gpu_ctx.construct_map_from_scans(mid, case["shape"], case["map_pose"], case["nodes"][:3])
        local = api.host_inverse_compound(case["map_pose"], node["pose"])
        seen = []
        for update in (False, True):
            if update:
                for nd in case["nodes"][3:]:
                    shape, _ = gpu_ctx.update_map_with_scan(mid, shape, case["map_pose"], nd)
            grid = gpu_ctx.download_level(mid, 0)
            geom = (shape["res"], shape["off_x"], shape["off_y"])
            q = dict(map_id=mid, geom=geom, angles=node["angles"], ranges=node["ranges"], rel_pose=node["rel_pose"],
                     init_pose=local)
            got, words = gpu_ctx.ray_check_batch([q], per_beam=True, **prm)
            want, want_words = R.ray_check(grid, geom, node["angles"], node["ranges"], node["rel_pose"], local, prm)
            assert R.strip(got[0]) == want
            assert np.array_equal(words[0], want_words)
            seen.append(want)
        assert seen[0] != seen[1]                           # the update changed what the rays cross
    finally:
        if gpu_ctx.has_grid(mid):
            gpu_ctx.release_grid(mid)
