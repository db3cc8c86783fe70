"""CPU suite of the free-space check of loop candidates: the whole-cell-move rule the floored reading rests on,
csm_host_ray_check against the numpy definition (tests/ray_check_reference.py) on every named case, the
threshold helper against the probability table, the refusals, what each named case exercises, and one case
with meaning (a scan at its true pose against a pose through the room's wall). Everything is an integer:
records and per-beam words are compared for equality."""
import ctypes as C
import math

import numpy as np
import pytest

import ray_check_reference as R
from csm_hip import _lib as L, api, synth

CASES = R.named_cases()
NAMES = [c["name"] for c in CASES]


@pytest.fixture(scope="module")
def references():
    return {c["name"]: R.check_case(c) for c in CASES}


@pytest.mark.parametrize("scale", [1, 2, 7, 100])
def test_whole_cell_move_moves_the_cells_and_nothing_else(oracle, scale):
    rng = np.random.RandomState(100 + scale)
    for _ in range(150):
        span = int(rng.choice([3, 40, 300])) * scale
        sx, sy, ex, ey = (int(v) for v in rng.randint(0, span, 4))
        if rng.rand() < 0.2:
            ex = sx + int(rng.randint(0, scale))          # one column, or nearly
        kx, ky = int(rng.randint(1, 50)), int(rng.randint(1, 50))
        base = oracle.ray_cells(sx, sy, ex, ey, scale)
        moved = oracle.ray_cells(sx + kx * scale, sy + ky * scale, ex + kx * scale, ey + ky * scale, scale)
        assert [(int(x) + kx, int(y) + ky) for x, y in base] == [(int(x), int(y)) for x, y in moved]
        assert len(set(base)) == len(base)                # no walk holds a cell twice


def test_named_cases_are_small_and_distinct():
    assert len(set(NAMES)) == len(NAMES)
    for c in CASES:
        assert c["grid"].shape[0] <= 80 and c["grid"].shape[1] <= 96
    assert any(c["grid"].shape[1] == 67 for c in CASES)
    assert {c["angles"].size for c in CASES} >= {1, 63, 65, 1081}
    assert {c["params"]["subpixel_scale"] for c in CASES} >= {1, 7, 100}
    assert {c["params"]["end_tolerance"] for c in CASES} >= {0, 1, 3}


@pytest.mark.parametrize("name", NAMES)
def test_named_case_exercises_what_it_aims_at(references, name):
    c = CASES[NAMES.index(name)]
    rec, words = references[name]
    assert c["aims"](rec), rec
    if c["walk"] is not None:
        assert c["walk"](R.beam_walks(c["geom"], c["angles"], c["ranges"], c["rel_pose"], c["pose"], c["params"]))
    assert rec["cells"] >= rec["cells_free"] + rec["cells_unknown"] + rec["cells_near"] + rec["cells_blocking"]
    assert (words == -2).sum() == rec["beams"] - rec["usable"] and (words == -1).sum() == rec["usable"] - rec["walked"]
    assert (words > 0).sum() == rec["blocked"] and max(0, int(words.max())) == rec["max_depth"]


def test_named_cases_cover_every_class_together(references):
    total = {k: sum(references[n][0][k] for n in NAMES) for k in R.FIELDS}
    assert all(total[k] > 0 for k in R.FIELDS), total
    other = sum(r["cells"] - r["cells_free"] - r["cells_unknown"] - r["cells_near"] - r["cells_blocking"]
                for r, _ in references.values())
    assert other > 0


@pytest.mark.parametrize("name", NAMES)
def test_host_restatement_equals_the_reference(references, name):
    c = CASES[NAMES.index(name)]
    want, want_words = references[name]
    got, words = api.host_ray_check(c["grid"], c["geom"], c["angles"], c["ranges"], c["rel_pose"], c["pose"],
                                    per_beam=True, **c["params"])
    assert got["host_beams"] == 0
    assert R.strip(got) == want
    assert np.array_equal(words, want_words)
    alone = api.host_ray_check(c["grid"], c["geom"], c["angles"], c["ranges"], c["rel_pose"], c["pose"],
                               **c["params"])
    assert alone == got                                    # per_beam = NULL


def test_threshold_values_against_the_probability_table():
    lut = api.host_probability_lut()
    for p_occ, p_free in ((0.65, 0.35), (0.5, 0.499), (0.9, 0.1), (lut[65535], lut[1]), (lut[2], lut[1]),
                          (lut[65535], lut[65534]), (0.7000001, 0.2999999)):
        occ, fre = api.host_ray_check_values(p_occ, p_free)
        assert 1 <= fre < occ <= 65535
        assert lut[occ] >= p_occ and (occ == 1 or lut[occ - 1] < p_occ)
        assert lut[fre] <= p_free and (fre == 65535 or lut[fre + 1] > p_free)
    assert api.host_ray_check_values(lut[65535], lut[1]) == (65535, 1)
    for bad in ((1.0, 0.3), (0.6, 0.0), (0.0, 0.001), (0.3, 0.6), (0.5, 0.5), (float("nan"), 0.3), (0.6, float("inf"))):
        with pytest.raises(api.CsmError) as e:
            api.host_ray_check_values(*bad)
        assert e.value.code == L.CSM_EINVAL


def test_argument_errors_are_einval():
    c = CASES[NAMES.index("horizontal")]

    def code(geom=c["geom"], pose=c["pose"], angles=c["angles"], **kw):
        try:
            api.host_ray_check(c["grid"], geom, angles, c["ranges"], c["rel_pose"], pose, **R.params(**kw))
        except api.CsmError as e:
            return e.code
        return 0

    assert code() == 0
    assert code(free_max=0) == L.CSM_EINVAL
    assert code(free_max=40000, occupied_min=40000) == L.CSM_EINVAL
    assert code(occupied_min=65536) == L.CSM_EINVAL
    assert code(subpixel_scale=0) == L.CSM_EINVAL
    assert code(subpixel_scale=L.RAY_CHECK_MAX_SCALE + 1) == L.CSM_EINVAL
    assert code(subpixel_scale=L.RAY_CHECK_MAX_SCALE) == 0
    assert code(end_tolerance=-1) == L.CSM_EINVAL
    assert code(scratch_limit_bytes=-1) == L.CSM_EINVAL
    assert code(usable_range_max=float("nan")) == L.CSM_EINVAL
    res = c["geom"][0]
    assert code(usable_range_max=res * 2.0 ** 20) == 0
    assert code(usable_range_max=res * 2.0 ** 20 * 1.0001) == L.CSM_EINVAL
    far = c["geom"][1] + res * 2.0 ** 20
    assert code(pose=(far, c["pose"][1], 0.0)) == 0
    assert code(pose=(far + 2 * res, c["pose"][1], 0.0)) == L.CSM_EINVAL
    assert code(pose=(c["pose"][0], c["geom"][2] - res * (2.0 ** 20 + 2), 0.0)) == L.CSM_EINVAL
    assert code(pose=(float("nan"), 0.0, 0.0)) == L.CSM_EINVAL
    assert code(geom=(0.0, 0.0, 0.0)) == L.CSM_EINVAL
    bad_angles = c["angles"].copy()
    bad_angles[0] = float("inf")
    assert code(angles=bad_angles) == L.CSM_EINVAL
    out = L.RayCheckResult()
    p = api.ray_check_params(**c["params"])
    assert L.load().csm_host_ray_check(None, 3, 3, C.byref(L.Geometry(*c["geom"])), None, None, C.byref(p),
                                       C.byref(out), None) == L.CSM_EINVAL


def test_true_pose_against_a_pose_through_the_wall(oracle):
    """The last scan of synth.map_case(2, n_scans=10, n_beams=360) on the oracle-built map of all ten, at its
    true pose and at a pose moved by 1.5 x the room's half width (make_room's, read off the generator's first
    wall segment) along the room's x axis: at least 0.5 half widths less its travel beyond the wall.
    Measured (occupied_min 40000, free_max 10000, end_tolerance 1): true pose blocked 9 of 359 walked (rate
    0.025); moved pose blocked 72 of 107 walked (rate 0.673)."""
    case = synth.map_case(2, n_scans=10, n_beams=360)
    shape, grid, _ = oracle.construct_map(case["shape"], case["map_pose"], case["nodes"])
    geom = (shape["res"], shape["off_x"], shape["off_y"])
    half_x = float(case["segs"][0][2])
    assert half_x > 0 and case["segs"][0][0] == -half_x
    node = case["nodes"][-1]
    moved_global = (node["pose"][0] + 1.5 * half_x, node["pose"][1], node["pose"][2])
    assert moved_global[0] > half_x + 1.0                   # beyond the wall
    prm = R.params(usable_range_min=node["min_range"], usable_range_max=node["max_range"])
    records = []
    for pose in (node["pose"], moved_global):
        local = api.host_inverse_compound(case["map_pose"], pose)
        want, words = R.ray_check(grid, geom, node["angles"], node["ranges"], node["rel_pose"], local, prm)
        got, got_words = api.host_ray_check(grid, geom, node["angles"], node["ranges"], node["rel_pose"], local,
                                            per_beam=True, **prm)
        assert R.strip(got) == want and np.array_equal(got_words, words)
        records.append(want)
    true, wrong = records
    print("true pose: blocked %d of %d walked; moved pose: blocked %d of %d walked"
          % (true["blocked"], true["walked"], wrong["blocked"], wrong["walked"]))
    assert true["walked"] > 0 and wrong["walked"] > 0
    assert true["blocked"] * wrong["walked"] < wrong["blocked"] * true["walked"]
