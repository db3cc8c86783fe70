"""Virtual scans on the host: csm_host_ray_cast (step by step, sequential) against the numpy / Python-integer
contract of tests/ray_cast_reference.py on every named case, in both directions, and on a seeded fuzz of a few
thousand rays; what each named case aims at; the sensor's cell as an end of every walk; dist2 and the ranges
against Python integers and math.sqrt; csm_host_ray_cast_min_dist2; every refusal. Records are integers:
everything is compared for equality."""
import math

import numpy as np
import pytest

import ray_cast_reference as RC
from csm_hip import _lib as L, api

CASES = RC.named_cases()
NAMES = [c["name"] for c in CASES]
FUZZ = RC.fuzz_cases()


def _host(c, **kw):
    return api.host_ray_cast(c["grid"], c["geom"], c["angles"], c["poses"], ranges=c["ranges"], **dict(c["params"], **kw))


@pytest.fixture(scope="module")
def references():
    return {c["name"]: RC.cast_case(c, with_walks=True) for c in CASES + FUZZ}


def test_the_cases_are_small_and_come_in_both_directions():
    assert len(set(NAMES)) == len(NAMES)
    for c in CASES:
        assert c["grid"].shape[0] <= 200 and c["grid"].shape[1] <= 160 and c["angles"].size <= 16
        assert (c["name"] + "_mirrored" in NAMES) != c["name"].endswith("_mirrored")


@pytest.mark.parametrize("name", NAMES)
def test_named_case(references, name):
    c = CASES[NAMES.index(name)]
    want, walks = references[name]
    assert c["aims"](c, want, walks), "the case misses its aim"
    got = _host(c)
    assert got.dtype == api.CAST_RECORD and got.shape == want.shape
    assert np.array_equal(got, want)


def test_mirrored_cases_walk_from_the_other_end(references):
    """Sensor at the low-x end: the reference's own order. At the high-x end: it swapped, the cast reverses."""
    swapped = {True: 0, False: 0}
    for c in CASES:
        for walks in references[c["name"]][1]:
            for w in walks:
                if w is not None and w["s"][0] != w["e"][0] and len({x for x, _ in w["cells"]}) > 1:
                    assert w["reversed"] == (w["s"][0] > w["e"][0])
                    swapped[w["reversed"]] += 1
    assert swapped[True] > 40 and swapped[False] > 40


def test_seeded_fuzz(references):
    rays = stopped = unknown = 0
    for c in FUZZ:
        want, walks = references[c["name"]]
        got = _host(c)
        assert np.array_equal(got, want), c["name"]
        rays += want.size
        stopped += int((want["kind"] == RC.OCCUPIED).sum())
        unknown += int((want["kind"] == RC.UNKNOWN).sum())
        # the sensor's cell is an end of every walk: the order of the definition exists
        assert all(w is None or w["sensor_is_an_end"] for ws in walks for w in ws), c["name"]
    assert rays >= 3000 and stopped > 500 and unknown > 100 and rays - stopped - unknown > 200


def test_dist2_and_ranges(references):
    for c in CASES + FUZZ:
        want, walks = references[c["name"]]
        scale, res = c["params"]["subpixel_scale"], c["geom"][0]
        got = _host(c)
        rng = api.host_ray_cast_ranges(got, res, scale, none_value=-1.0)
        assert rng.shape == got.shape
        for p in range(got.shape[0]):
            for i in range(got.shape[1]):
                r = got[p, i]
                if r["kind"] == RC.NONE:
                    assert rng[p, i] == -1.0 and r.tobytes() == bytes(24)
                    continue
                d2 = RC.dist2((int(r["cell_x"]), int(r["cell_y"])), walks[p][i]["s"], scale)
                assert int(r["dist2"]) == d2 < 2 ** 62
                assert rng[p, i] == (0.5 * (res / scale)) * math.sqrt(float(d2))
    assert api.host_ray_cast_ranges(np.zeros(0, api.CAST_RECORD), 0.05, 100).shape == (0,)
    big = np.zeros(1, api.CAST_RECORD)
    big[0] = (1, 2, 3, RC.OCCUPIED, 2 ** 61 + 12345)
    assert api.host_ray_cast_ranges(big, 0.05, 512)[0] == (0.5 * (0.05 / 512)) * math.sqrt(float(2 ** 61 + 12345))


def test_min_dist2():
    f = api.host_ray_cast_min_dist2
    assert f(0.0, 0.05, 100) == 0
    assert f(0.25, 0.25, 100) == 200 ** 2
    assert f(0.25 + 1e-9, 0.25, 100) == 201 ** 2
    for rm, res, scale in [(0.3, 0.05, 100), (1.234, 0.07, 7), (19.99, 0.25, 1), (5.0, 0.05, 512)]:
        assert f(rm, res, scale) == RC.min_dist2(rm, res, scale) == int(math.ceil(2.0 * rm / (res / scale))) ** 2
    assert f(1e300, 0.05, 100) == f(math.inf, 0.05, 100) == 2 ** 62
    for bad in [(-1e-9, 0.05, 100), (math.nan, 0.05, 100), (1.0, 0.0, 100), (1.0, math.inf, 100), (1.0, 0.05, 0),
                (1.0, 0.05, L.RAY_CHECK_MAX_SCALE + 1)]:
        with pytest.raises(api.CsmError) as e:
            f(*bad)
        assert e.value.code == L.CSM_EINVAL


def test_range_min_that_nothing_reaches():
    c = CASES[NAMES.index("horizontal")]
    assert set(_host(c, range_min=math.inf)["kind"].reshape(-1).tolist()) == {RC.NONE}


def test_empty_inputs_are_valid():
    c = CASES[NAMES.index("horizontal")]
    assert api.host_ray_cast(c["grid"], c["geom"], [], c["poses"], **c["params"]).shape == (1, 0)
    assert api.host_ray_cast(c["grid"], c["geom"], c["angles"], np.zeros((0, 3)), **c["params"]).shape == (0, 2)


REFUSALS = [
    ("scale_0", dict(subpixel_scale=0), {}),
    ("scale_above_max", dict(subpixel_scale=L.RAY_CHECK_MAX_SCALE + 1), {}),
    ("occupied_min_0", dict(occupied_min=0), {}),
    ("occupied_min_65536", dict(occupied_min=65536), {}),
    ("unknown_stops_2", dict(unknown_stops=2), {}),
    ("scratch_negative", dict(scratch_limit_bytes=-1), {}),
    ("range_max_0", dict(range_max=0.0), {}),
    ("range_max_negative", dict(range_max=-1.0), {}),
    ("range_max_inf", dict(range_max=math.inf), {}),
    ("range_max_nan", dict(range_max=math.nan), {}),
    ("range_max_too_many_cells", dict(range_max=RC.RES * (2 ** 20 + 1)), {}),
    ("range_min_negative", dict(range_min=-0.001), {}),
    ("range_min_nan", dict(range_min=math.nan), {}),
    ("angle_nan", {}, dict(angles=[0.0, math.nan])),
    ("angle_inf", {}, dict(angles=[math.inf, 0.0])),
    ("pose_nan", {}, dict(poses=[[0.0, math.nan, 0.0]])),
    ("pose_theta_inf", {}, dict(poses=[[0.0, 0.0, math.inf]])),
    ("sensor_too_far_x", {}, dict(poses=[[RC.GEOM[1] + RC.RES * (2 ** 20 + 1), 0.0, 0.0]])),
    ("sensor_too_far_y", {}, dict(poses=[[0.0, RC.GEOM[2] - RC.RES * (2 ** 20 + 1), 0.0]])),
    ("resolution_0", {}, dict(geom=(0.0, 0.0, 0.0))),
    ("resolution_nan", {}, dict(geom=(math.nan, 0.0, 0.0))),
    ("offset_inf", {}, dict(geom=(0.25, math.inf, 0.0))),
]


@pytest.mark.parametrize("name", [r[0] for r in REFUSALS])
def test_refusals(name):
    _, prm, args = REFUSALS[[r[0] for r in REFUSALS].index(name)]
    c = dict(CASES[NAMES.index("horizontal")], **args)
    with pytest.raises(api.CsmError) as e:
        api.host_ray_cast(c["grid"], c["geom"], c["angles"], c["poses"], ranges=c["ranges"], **dict(c["params"], **prm))
    assert e.value.code == L.CSM_EINVAL


def test_refusals_of_the_c_entry():
    """Null pointers and negative counts, which the Python wrapper never passes."""
    import ctypes as C
    lib = L.load()
    c = CASES[NAMES.index("horizontal")]
    g = c["grid"]
    sc, keep = api._cast_scan(c["angles"], None)
    geom, prm = L.Geometry(*c["geom"]), api.ray_cast_params(**c["params"])
    poses = np.ascontiguousarray(c["poses"])
    out = np.zeros((1, 2), api.CAST_RECORD)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(grid=ptr(g), rows=g.shape[0], cols=g.shape[1], geom=C.byref(geom), scan=C.byref(sc), poses=ptr(poses), n=1,
             prm=C.byref(prm), out=ptr(out)):
        return lib.csm_host_ray_cast(grid, rows, cols, geom, scan, poses, n, prm, out)

    assert call() == L.CSM_OK
    for kw in (dict(grid=None), dict(rows=0), dict(cols=0), dict(geom=None), dict(scan=None), dict(poses=None),
               dict(n=-1), dict(prm=None), dict(out=None)):
        assert call(**kw) == L.CSM_EINVAL, kw
    bad = L.Scan()
    bad.n_points = 2                       # angles null
    assert call(scan=C.byref(bad)) == L.CSM_EINVAL
    bad.n_points = -1
    assert call(scan=C.byref(bad)) == L.CSM_EINVAL
    assert call(n=0, poses=None, out=None) == L.CSM_OK
    assert lib.csm_host_ray_cast_ranges(None, 1, 0.05, 100, 0.0, ptr(out)) == L.CSM_EINVAL
    assert lib.csm_host_ray_cast_ranges(ptr(out), -1, 0.05, 100, 0.0, ptr(out)) == L.CSM_EINVAL
    assert lib.csm_host_ray_cast_ranges(ptr(out), 1, 0.0, 100, 0.0, ptr(out)) == L.CSM_EINVAL
    assert lib.csm_host_ray_cast_ranges(ptr(out), 1, 0.05, 0, 0.0, ptr(out)) == L.CSM_EINVAL
    assert lib.csm_host_ray_cast_min_dist2(1.0, 0.05, 100, None) == L.CSM_EINVAL


def test_the_edge_case_has_ends_on_edges():
    for name in ("ends_on_cell_edges", "ends_on_cell_edges_mirrored"):
        c = CASES[NAMES.index(name)]
        assert RC.ends_on_edges(c) >= 3
