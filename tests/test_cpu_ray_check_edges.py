"""CPU suite of the ray check's edge cases (tests/ray_check_reference.py): the windowed reference in Python
integers against the step-by-step oracle; far frames up to the documented 2^20-cell bound, where the closed
form's products pass 2^55; rays clipped at every edge of the map; cell values on the thresholds; a seeded
sweep. Each group states on the reference alone what it exercises, and csm_host_ray_check (64-bit C++, step
by step) equals the reference on every case. Everything is an integer: records and words are compared for
equality."""
import math

import numpy as np
import pytest

import ray_check_reference as R
from csm_hip import api

NAMED = R.named_cases()
FAR = R.far_cases()
CLIP = R.clip_cases()
THRESHOLD = R.threshold_cases()


def _names(cases):
    return [c["name"] for c in cases]


def _host(c):
    got, words = api.host_ray_check(c["grid"], c["geom"], c["angles"], c["ranges"], c["rel_pose"], c["pose"],
                                    per_beam=True, **c["params"])
    assert got["host_beams"] == 0
    return R.strip(got), words


def _same(got, want):
    assert got[0] == want[0]
    assert np.array_equal(got[1], want[1])


# ---- the windowed reference ----

def _random_rays(scale, count, seed):
    rng = np.random.RandomState(seed)
    for k in range(count):
        span = int(rng.choice([2, 3, 40, 300])) * scale
        sx, sy, ex, ey = (int(v) for v in rng.randint(0, span, 4))
        kind = k % 8
        if kind == 0:
            ex = sx - sx % scale + int(rng.randint(0, scale))            # one column
        elif kind in (1, 2):                                               # through exact cell corners
            n = int(rng.randint(1, max(2, span // scale)))
            up = 1 if kind == 1 else -1
            fx = int(rng.randint(0, scale))
            sx = sx - sx % scale + fx
            sy = sy - sy % scale + (fx if up > 0 else scale - 1 - fx) + (n * scale if up < 0 else 0)
            ex, ey = sx + n * scale, sy + up * n * scale
            if rng.rand() < 0.5:
                sx, sy, ex, ey = ex, ey, sx, sy
        yield sx, sy, ex, ey


@pytest.mark.parametrize("scale", [1, 2, 3, 7, 100, 512])
def test_window_cells_equals_the_oracle_walk(oracle, scale):
    count, corners = 0, 0
    for sx, sy, ex, ey in _random_rays(scale, 1800, 500 + scale):
        walk = [(int(x), int(y)) for x, y in oracle.ray_cells(sx, sy, ex, ey, scale)]
        cells = R.window_cells(sx, sy, ex, ey, scale, 0, 1 << 40, 0, 1 << 40)
        assert len(set(cells)) == len(cells), (sx, sy, ex, ey)
        assert set(cells) == set(walk) and len(cells) == len(walk), (sx, sy, ex, ey)
        corners += any(a[0] != b[0] and a[1] != b[1] for a, b in zip(walk, walk[1:]))
        # a window cuts the same cells out, whichever way the ends are given
        c_lo, c_hi, r_lo, r_hi = 1, max(sx, ex) // scale - 1, 2, max(sy, ey) // scale - 1
        want = {(x, y) for x, y in walk if c_lo <= x <= c_hi and r_lo <= y <= r_hi}
        assert set(R.window_cells(ex, ey, sx, sy, scale, c_lo, c_hi, r_lo, r_hi)) == want
        count += 1
    assert count == 1800 and corners >= 200                # 6 scales: 10,800 rays


def test_windowed_check_equals_the_full_walk_on_every_named_case():
    for c in NAMED + CLIP + THRESHOLD:
        _same(R.check_case_windowed(c), R.check_case(c))


# ---- far frames ----

@pytest.fixture(scope="module")
def far_references():
    return {c["name"]: R.check_case_windowed(c) for c in FAR}


def test_far_cases_reach_the_documented_bound_and_stay_inside_it():
    assert len(set(_names(FAR))) == len(FAR)
    assert {c["params"]["subpixel_scale"] for c in FAR} == {1, 100, 512}
    products = {c["name"]: R.largest_case_product(c) for c in FAR}
    for c in FAR:
        assert c["grid"].shape[0] <= 40 and c["grid"].shape[1] <= 48 and c["angles"].size <= 8
        assert 2 ** c["product_bits"] <= products[c["name"]] < 2 ** 63 or c["product_bits"] == 0, products[c["name"]]
        res, off_x, off_y = c["geom"]
        S = api.host_compound(c["pose"], c["rel_pose"])
        assert max(abs(S[0] - off_x), abs(S[1] - off_y)) / res <= 2 ** 20
        assert c["params"]["usable_range_max"] / res <= 2 ** 20
    assert max(products.values()) < 2 ** 63
    assert sum(p > 2 ** 55 for p in products.values()) >= 3      # the oblique rays at scale 512
    print("largest product: 2^%.2f" % math.log2(max(products.values())))
    # sensors at +-(2^20 - 3) cells on each axis, rays of just under 2^20 cells
    cells = {(round((c["pose"][0] - R.GEOM[1]) / R.RES - 0.5), round((c["pose"][1] - R.GEOM[2]) / R.RES - 0.5))
             for c in FAR if c["geom"] == R.GEOM}
    n = R.FAR_CELLS - 3
    assert {(n, 20), (-n, 20), (20, n), (20, -n)} <= cells
    assert any(c["ranges"].max() == (R.FAR_CELLS - 5) * R.RES for c in FAR)


@pytest.mark.parametrize("name", _names(FAR))
def test_far_case_exercises_what_it_aims_at(far_references, name):
    c = FAR[_names(FAR).index(name)]
    rec, words = far_references[name]
    print(name, rec, "largest product 2^%.1f" % math.log2(max(R.largest_case_product(c), 1)))
    assert c["aims"](rec), rec
    assert (words == -2).sum() == rec["beams"] - rec["usable"] and (words == -1).sum() == rec["usable"] - rec["walked"]
    assert (words > 0).sum() == rec["blocked"] and max(0, int(words.max())) == rec["max_depth"]


@pytest.mark.parametrize("name", _names(FAR))
def test_host_restatement_equals_the_windowed_reference_far_out(far_references, name):
    _same(_host(FAR[_names(FAR).index(name)]), far_references[name])


# ---- clip edges ----

@pytest.mark.parametrize("name", _names(CLIP))
def test_clip_case_exercises_what_it_aims_at_and_the_host_equals_it(name):
    c = CLIP[_names(CLIP).index(name)]
    assert c["grid"].shape in ((17, 23), (70, 65), (3, 129))
    rec, words = R.check_case(c)
    print(name, rec)
    assert c["aims"](rec), rec
    if c["walk"] is not None:
        assert c["walk"](R.case_walks(c))
    res, off_x, off_y = c["geom"]
    assert -300 <= (c["pose"][0] - off_x) / res <= 300 and -300 <= (c["pose"][1] - off_y) / res <= 300
    _same(_host(c), (rec, words))


def test_clip_cases_name_every_direction():
    names = _names(CLIP)
    assert len(set(names)) == len(names)
    fans = [n for n in names if n.startswith("clip_fan_from_")]
    assert len(fans) == 8 and all(CLIP[names.index(n)]["angles"].size == 24 for n in fans)


# ---- threshold values ----

def test_threshold_cases_put_every_value_in_every_class():
    assert len(THRESHOLD) == 6 and all(c["angles"].size == 90 for c in THRESHOLD)
    for fm, om in R.THRESHOLDS:
        cases = [c for c in THRESHOLD if (c["params"]["free_max"], c["params"]["occupied_min"]) == (fm, om)]
        assert sorted(c["params"]["end_tolerance"] for c in cases) == [0, 2]
        total = dict.fromkeys(R.FIELDS, 0)
        other = 0
        for c in cases:
            assert set(np.unique(c["grid"]).tolist()) == set(R.threshold_values(fm, om))
            rec, words = R.check_case(c)
            print(c["name"], rec)
            assert c["aims"](rec), rec
            _same(_host(c), (rec, words))
            for k in R.FIELDS:
                total[k] += rec[k]
            other += R.other_cells(rec)
        for k in ("cells_unknown", "cells_free", "cells_near", "cells_blocking", "end_free", "end_occupied", "end_unknown"):
            assert total[k] > 0, (fm, om, k)
        end_none = total["end_inside"] - total["end_free"] - total["end_occupied"] - total["end_unknown"]
        if om == fm + 1:                                    # no value lies between the thresholds
            assert other == 0 and end_none == 0
        else:
            assert other > 0 and end_none > 0


def test_threshold_values_land_on_the_side_the_definition_says():
    """One beam along a row that holds the cycle and ends beyond the map, counted straight from the
    definition: 0 unknown, 1 .. free_max free, free_max + 1 .. occupied_min - 1 other, occupied_min .. 65535
    occupied (and blocking: the hit cell is outside, the tolerance 0)."""
    for fm, om in R.THRESHOLDS:
        missed = R.threshold_values(fm, om) + [1]                       # 1 x 9; the sensor in the last cell
        grid = np.array([missed], np.uint16)
        x, y = R._at(8, 0)
        prm = R.params(free_max=fm, occupied_min=om, end_tolerance=0)
        got = api.host_ray_check(grid, R.GEOM, [math.pi], [9.2 * R.RES], (0.0, 0.0, 0.0), (x, y, 0.0), **prm)
        want = R.ray_check(grid, R.GEOM, [math.pi], [9.2 * R.RES], (0.0, 0.0, 0.0), (x, y, 0.0), prm)[0]
        assert R.strip(got) == want
        assert got["cells"] == 9 and got["end_inside"] == 0
        assert got["cells_unknown"] == sum(v == 0 for v in missed)
        assert got["cells_free"] == sum(0 < v <= fm for v in missed)
        assert got["cells_blocking"] == sum(v >= om for v in missed)
        assert R.other_cells(got) == sum(fm < v < om for v in missed)


# ---- bookkeeping cases (the GPU suite runs them; here: that the reference does what they are for) ----

def test_bookkeeping_cases_are_what_the_gpu_suite_expects():
    cases = R.bookkeeping_cases()
    assert [c["angles"].size for c in cases] == R.BOOKKEEPING_COUNTS
    assert {c["grid_index"] for c in cases} == {0, 1, 2}
    for c in cases + R.late_switch_cases() + [R.edge_fan_case(64)]:
        rec, words = R.check_case(c)
        assert c["aims"](rec), (c["name"], rec)
        _same(_host(c), (rec, words))


# ---- the sweep ----

@pytest.fixture(scope="module")
def sweep():
    return {seed: R.sweep_cases(seed) for seed in R.SWEEP_SEEDS}


def test_sweep_draws_what_it_says(sweep):
    sets = set()
    for seed, cases in sweep.items():
        assert len(cases) == 48 and len({c["grid_index"] for c in cases}) == 6
        assert len({tuple(sorted(c["params"].items())) for c in cases}) == 1
        p = cases[0]["params"]
        sets.add((p["subpixel_scale"], p["end_tolerance"], p["free_max"], p["occupied_min"]))
        for c in cases:
            assert c["grid"].shape[0] in R.SWEEP_ROWS and c["grid"].shape[1] in R.SWEEP_COLS
            assert c["angles"].size in R.SWEEP_BEAMS
            usable = c["ranges"][(c["ranges"] > 0.01) & (c["ranges"] < 31.0)] / c["geom"][0]
            assert usable.size == 0 or (usable.min() >= 0.5 and usable.max() <= 120.0 + 1e-9)
            res, off_x, off_y = c["geom"]
            col, row = (c["pose"][0] - off_x) / res, (c["pose"][1] - off_y) / res
            assert -200 <= col <= c["grid"].shape[1] + 200 and -200 <= row <= c["grid"].shape[0] + 200
        assert sum(c["geom"] == R.GEOM for c in cases) == 24
    assert {s[0] for s in sets} == {1, 2, 3, 37, 100, 512} and {s[1] for s in sets} == {0, 1, 2, 5}
    assert {s[2:] for s in sets} == set(R.THRESHOLDS)


def test_sweep_covers_every_field_side_and_crossing_and_the_host_equals_it(sweep):
    total = dict.fromkeys(R.FIELDS, 0)
    other = crossing = untouched = 0
    entered = {"low_x": 0, "high_x": 0, "low_y": 0, "high_y": 0}
    for seed, cases in sweep.items():
        for c in cases:
            rec, words = R.check_case(c)
            _same(_host(c), (rec, words))
            for k in R.FIELDS:
                total[k] += rec[k]
            other += R.other_cells(rec)
            untouched += int((words == -1).sum())
            rows, cols = c["grid"].shape
            scale = c["params"]["subpixel_scale"]
            for w in R.case_walks(c):
                if w is None or R._outside(w["s"], scale, (rows, cols)) == (0, 0):
                    continue
                path = w["cells"] if w["s"][0] <= w["e"][0] else w["cells"][::-1]      # from the sensor on
                inside = [0 <= x < cols and 0 <= y < rows for x, y in path]
                if True not in inside:
                    continue
                x, y = path[inside.index(True) - 1]                                    # the last cell before the map
                side = "low_x" if x < 0 else "high_x" if x >= cols else "low_y" if y < 0 else "high_y"
                entered[side] += 1
                crossing += R._outside(w["e"], scale, (rows, cols)) != (0, 0)
    print(total, "other", other, "entered", entered, "crossing", crossing, "untouched", untouched)
    assert all(total[k] > 0 for k in R.FIELDS), total
    assert other > 0
    assert all(n > 0 for n in entered.values()), entered
    assert crossing > 0
    assert untouched > 0


# ---- what the far cases ask of the device's arithmetic ----

def _wrapped(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def _c_div(a, b):
    q = abs(a) // abs(b)                                    # C's division truncates
    return q if (a < 0) == (b < 0) else -q


def _closed_form_cells(sx, sy, ex, ey, scale, clip, bits):
    """ray_cells_closed_form<true> of csm_map.hpp, statement by statement, with every `long long` held in
    `bits` bits and every (int) cast in 32: which cells the device's text names if its wide integers were
    that wide. Lanes and the spreading of cells over them are left out: they choose who visits, not what."""
    w = lambda v: _wrapped(v, bits)
    i32 = lambda v: _wrapped(v, 32)
    x_lo, x_hi, y_lo, y_hi = clip
    if sx > ex:
        sx, sy, ex, ey = ex, ey, sx, sy
    x0, y0, x1, y1 = sx // scale, sy // scale, ex // scale, ey // scale
    if x0 == x1:
        if x0 < x_lo or x0 > x_hi:
            return []
        return [(x0, y) for y in range(max(min(y0, y1), y_lo), min(max(y0, y1), y_hi) + 1)]
    dx, dy = ex - sx, ey - sy
    den = w(2 * scale * dx)
    n0 = w(w(y0 * den) + w((2 * (sy % scale) + 1) * dx))
    first, last = 2 * scale - (2 * (sx % scale) + 1), 2 * (ex % scale) + 1
    m = x1 - x0
    out = []
    for j in range(max(0, x_lo - x0), min(m, x_hi - x0) + 1):
        n_out = w(n0 + w(dy * w(first + 2 * scale * j))) if j < m else \
            w(n0 + w(dy * w(first + 2 * scale * (m - 1) + last)))
        n_in = w(n0 + w(dy * w(first + 2 * scale * (j - 1))))
        if den == 0:
            return None                                     # the narrow form cannot even divide
        if dy > 0:
            lo = y0 if j == 0 else i32(_c_div(n_in, den))
            hi = i32(_c_div(w(n_out + den - 1), den)) - 1
        else:
            hi = y0 if j == 0 else i32(_c_div(w(n_in + den - 1), den)) - 1
            lo = i32(_c_div(n_out, den))
        out += [(x0 + j, y) for y in range(max(lo, y_lo), min(hi, y_hi) + 1)]
    return out


def _device_text_agrees(c, bits):
    """Per usable beam of the case: do the device's statements at `bits` bits name the reference's cells?"""
    rows, cols = c["grid"].shape
    scale = c["params"]["subpixel_scale"]
    same = []
    for w in R.case_ends(c):
        if w is None:
            continue
        (sx, sy), (ex, ey) = w["s"], w["e"]
        bx, by = min(sx, ex) // scale, min(sy, ey) // scale
        ray = (sx - bx * scale, sy - by * scale, ex - bx * scale, ey - by * scale, scale)
        clip = (-bx, cols - 1 - bx, -by, rows - 1 - by)
        got = _closed_form_cells(*ray, clip, bits)
        same.append(got is not None and sorted(got) == sorted(R.window_cells(*ray, *clip)))
    return same


def test_far_cases_need_the_64_bits_and_64_bits_are_enough():
    """The closed form as csm_map.hpp writes it (truncating divisions, ceilings as (n + den - 1) / den) equals
    the reference on every far and clip case when its wide integers hold 64 bits. Held in 32 bits it names
    other cells on every far case at scale 512 that reaches the map (den = 2 scale dx alone passes 2^31
    there): these inputs tell the two apart, which no case at ordinary distances does."""
    for c in FAR + CLIP:
        assert all(_device_text_agrees(c, 64)), c["name"]
    for c in CLIP:
        assert all(_device_text_agrees(c, 32)), c["name"]   # ordinary distances: 32 bits would have passed
    narrow = {c["name"]: _device_text_agrees(c, 32) for c in FAR}
    told_apart = [n for n, same in narrow.items() if not all(same)]
    print("far cases that 32-bit arithmetic gets wrong: %d of %d" % (len(told_apart), len(FAR)))
    for c in FAR:
        if c["params"]["subpixel_scale"] == 512 and "miss" not in c["name"]:
            assert c["name"] in told_apart
