"""CPU suite of the distance fields (no GPU): every claim a case of tests/distance_reference.py is chosen for,
proved on the numpy statement, so that a GPU failure cannot be a badly made case; and the three host
functions (csm_host_distance_transform, csm_host_distance_map, csm_host_distance_kernel) against the numpy
statement on every case. Bar: equality of integers; nothing has a tolerance."""
import math

import numpy as np
import pytest

import distance_reference as DR
from csm_hip import _lib as Lb, api


def _at(name, r, c, occupied_min=32768):
    g, d2, nearest = DR.expected(name, occupied_min)
    return int(d2[r, c]), int(nearest[r, c])


def test_tie_cases_are_ties_and_the_smallest_index_wins():
    # the cross: four obstacles 5 away from the centre, (0, 5) has the smallest index
    assert _at("cross", 5, 5) == (25, 0 * 11 + 5)
    # 3-4-5: five obstacles 5 away from (5, 5), found in four different columns and three different rows
    for r, c in DR.PYTHAGORAS:
        assert (r - 5) ** 2 + (c - 5) ** 2 == 25
    assert _at("pythagoras", 5, 5) == (25, 2 * 12 + 1) and 2 * 12 + 1 == 25
    assert _at("tie_column", 4, 2) == (9, 1 * 5 + 2)            # above and below: the upper one
    assert _at("tie_row", 2, 4) == (9, 2 * 9 + 1)               # left and right: the left one
    # where a row search that stops at k^2 >= best goes wrong: an obstacle of the cell's own row at k^2 == best
    # with the smaller index. (5, 7) of own_row_tie is 5 from (8, 3) [met at k = 4] and from (5, 2) [k = 5]
    assert (8 - 5) ** 2 + (3 - 7) ** 2 == 25 == (7 - 2) ** 2
    assert _at("own_row_tie", 5, 7) == (25, 5 * 11 + 2)


def test_degenerate_cases_are_what_they_are_named():
    assert _at("one_cell", 0, 0) == (0, 0)
    assert _at("one_cell_free", 0, 0) == (DR.NONE, DR.NONE)
    for name in ("no_obstacle", "one_cell_free"):
        g, d2, nearest = DR.expected(name)
        assert (d2 == DR.NONE).all() and (nearest == DR.NONE).all()
    g, d2, nearest = DR.expected("all_obstacle")
    assert (d2 == 0).all() and np.array_equal(nearest.reshape(-1), np.arange(g.size))
    g = DR.grid_of("max_value")
    assert int((g == 65535).sum()) == 2 and int((g >= 32768).sum()) > 2
    _, d2, nearest = DR.expected("max_value", 65535)
    assert set(np.unique(nearest).tolist()) == {7 * 40 + 9, 20 * 40 + 33}
    assert (DR.expected("max_value", 70000)[1] == DR.NONE).all()
    assert DR.grid_of("line1x200").shape == (1, 200) and DR.grid_of("line200x1").shape == (200, 1)


def test_seam_cases_cross_every_boundary_of_the_row_pass():
    for n in DR.LAST_COLUMN:
        g, d2, nearest = DR.expected("last_column%d" % n)
        rr, cc = np.nonzero(g >= 32768)
        assert set(cc.tolist()) == {n - 1} and g.shape[0] > DR.RUN_ROWS
        assert int(d2[0, 0]) == (n - 1) ** 2                    # the first lane walks the whole row
    g, d2, nearest = DR.expected("tall_last_row")
    assert g.shape[0] > 4 * DR.RUN_ROWS and np.nonzero(g >= 32768)[0].tolist() == [g.shape[0] - 1]
    assert int(d2[0, 4]) == (g.shape[0] - 1) ** 2
    g, d2, nearest = DR.expected("wide")
    assert g.shape[1] > DR.WIDE_COLS and g.shape[0] > DR.RUN_ROWS and len(np.unique(nearest)) == 3
    # staged rows beyond 64 KB, in both forms of the row pass; `wide` stays well below
    assert DR.grid_of("wide_four_rows").shape == (DR.RUN_ROWS + 1, DR.WIDE_COLS)
    assert DR.grid_of("widest").shape[1] == DR.MAX_SIDE
    assert DR.staged_bytes(DR.WIDE_COLS) == DR.staged_bytes(DR.MAX_SIDE) == 65552 > 64 * 1024
    assert DR.staged_bytes(DR.grid_of("wide").shape[1]) < 64 * 1024
    assert int(DR.expected("widest")[1][1, 0]) == 1 and int(DR.expected("widest")[1].max()) < 2 ** 31
    top, bottom = DR.expected("tallest_top")[1], DR.expected("tallest_bottom")[1]
    assert int(top[-1, 0]) == int(bottom[0, 0]) == 32766 ** 2 and top.shape == (DR.MAX_SIDE, 1)
    for name in ("pad70", "pad130"):
        assert DR.grid_of(name).shape[1] % 8 != 0               # pitch > cols
    for name, density in zip(DR.RANDOM_CASES, DR.DENSITIES * 3):
        g = DR.grid_of(name)
        assert abs(float((g >= 32768).mean()) - density) < 0.4 * density + 0.002


def test_clamp_cases_hold_the_cells_around_the_radius():
    g, d2, _ = DR.expected("far200")
    assert int(d2[0, 0]) == 79202 and int((d2 > 255 * 255).sum()) == 765
    g, d2, _ = DR.expected("clamp2x300")
    have = set(np.unique(d2).tolist())
    for R in DR.CLAMP_RADII:
        assert R * R in have and R * R + 1 in have
        # R^2 - 1 = (R - 1)(R + 1) is a sum of two squares for R = 1 only among these radii: the cell below
        # the radius is the one with the largest d2 < R^2 instead
        two_squares = any(math.isqrt(R * R - 1 - a * a) ** 2 == R * R - 1 - a * a for a in range(R))
        assert two_squares == (R == 1)
        assert max(v for v in have if v < R * R) >= (R - 1) ** 2
    ramp = DR.table_of("ramp", 255)
    assert len(set(ramp.tolist())) == ramp.size and int(ramp.min()) > 0     # a wrong index shows


def test_low_known_case():
    g = DR.grid_of("low_known")
    assert DR.first_known(g) == (9, 11)
    for R, kind, keep, want in [(3, "gauss", False, (0, 0)), (3, "gauss", True, (9, 11)), (3, "zeros", False, g.shape)]:
        out = DR.distance_map(g, DR.table_of(kind, R), R, keep_unknown=keep)
        assert DR.first_known(out) == want
    # T[R^2] = 0: the first row / column within R of an obstacle
    t = DR.table_of("cut", 3)
    assert int(t[9]) == 0 and int(t[8]) > 0
    out = DR.distance_map(g, t, 3)
    d2 = DR.expected("low_known")[1]
    rr, cc = np.nonzero(d2 < 9)
    assert DR.first_known(out) == (int(rr.min()), int(cc.min())) and DR.first_known(out) != (0, 0)


def test_table_expression_matches_math_exp():
    for sigma, res, R, peak, floor_value in [(0.25, 0.05, 15, 65534, 1), (1.0, 0.05, 60, 65534, 1),
                                             (0.5, 0.025, 255, 40000, 0), (0.1, 0.05, 6, 7, 7)]:
        got = api.host_distance_kernel(sigma, res, R, peak, floor_value)
        assert got.dtype == np.uint16 and np.array_equal(got, DR.kernel(sigma, res, R, peak, floor_value))
        assert int(got[0]) == peak and (np.diff(got.astype(np.int64)) <= 0).all()
    for bad in [(0.0, 0.05, 3, 65534, 1), (0.1, 0.05, 0, 65534, 1), (0.1, 0.05, 256, 65534, 1),
                (0.1, 0.05, 3, 65535, 1), (0.1, 0.05, 3, 10, 11), (float("nan"), 0.05, 3, 65534, 1)]:
        t = np.zeros(256 * 256, np.uint16)
        assert Lb.load().csm_host_distance_kernel(*bad, t.ctypes.data) == Lb.CSM_EINVAL


@pytest.mark.parametrize("name,occupied_min", DR.CASES)
def test_host_transform_equals_the_definition(name, occupied_min):
    g, d2, nearest = DR.expected(name, occupied_min)
    got_d2, got_nearest = api.host_distance_transform(g, occupied_min)
    assert np.array_equal(got_d2, d2), np.argwhere(got_d2 != d2)[:8]
    assert np.array_equal(got_nearest, nearest), np.argwhere(got_nearest != nearest)[:8]


@pytest.mark.parametrize("keep_unknown", [False, True])
@pytest.mark.parametrize("name,R,kind,occupied_min", DR.FIELD_CASES)
def test_host_map_equals_the_definition(name, R, kind, occupied_min, keep_unknown):
    g, t, want = DR.field_expected(name, R, kind, occupied_min, keep_unknown)
    got = api.host_distance_map(g, radius=R, occupied_min=occupied_min, keep_unknown=keep_unknown, table=t)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]


def test_host_functions_refuse_what_the_header_lists():
    lib = Lb.load()
    g = np.full((4, 5), 40000, np.uint16)
    out16, out32 = np.zeros((4, 5), np.uint16), np.zeros((4, 5), np.uint32)
    t = DR.table_of("ramp", 2)
    over = t.copy()
    over[3] = 65535
    ptr = lambda a: a.ctypes.data
    assert lib.csm_host_distance_transform(ptr(g), 4, 5, 32768, None, None) == Lb.CSM_EINVAL
    assert lib.csm_host_distance_transform(ptr(g), 4, 5, 0, ptr(out32), None) == Lb.CSM_EINVAL
    assert lib.csm_host_distance_transform(ptr(g), 0, 5, 32768, ptr(out32), None) == Lb.CSM_EINVAL
    assert lib.csm_host_distance_transform(ptr(g), 4, 32768, 32768, ptr(out32), None) == Lb.CSM_EINVAL
    assert lib.csm_host_distance_transform(ptr(g), 4, 5, 32768, ptr(out32), None) == 0 and (out32 == 0).all()
    assert lib.csm_host_distance_transform(ptr(g), 4, 5, 32768, None, ptr(out32)) == 0
    assert np.array_equal(out32.reshape(-1), np.arange(20))
    for radius, table, occ in [(0, t, 32768), (256, t, 32768), (2, over, 32768), (2, t, 0), (2, None, 32768)]:
        p = Lb.DistanceParams(radius, occ, 0, 0, None if table is None else ptr(table))
        assert lib.csm_host_distance_map(ptr(g), 4, 5, p, ptr(out16)) == Lb.CSM_EINVAL
    p = Lb.DistanceParams(2, 32768, 0, 0, ptr(t))
    assert lib.csm_host_distance_map(ptr(g), 32768, 5, p, ptr(out16)) == Lb.CSM_EINVAL
    assert lib.csm_host_distance_map(ptr(g), 4, 5, p, ptr(out16)) == 0 and (out16 == t[0]).all()


def test_host_transform_of_a_large_map_is_not_brute_force():
    """2000 x 2000 (the largest map of the benchmark's configs) in seconds, with obstacles or without."""
    rng = np.random.default_rng(5)
    g = np.zeros((2000, 2000), np.uint16)
    d2, nearest = api.host_distance_transform(g)
    assert (d2 == DR.NONE).all() and (nearest == DR.NONE).all()
    # a wall along the far row: an obstacle in every column, each about 2000 cells away
    g[1999, :] = 50000
    d2, nearest = api.host_distance_transform(g)
    rows = np.arange(2000, dtype=np.int64)[:, None]
    assert np.array_equal(d2, np.broadcast_to((1999 - rows) ** 2, g.shape))
    assert np.array_equal(nearest, np.broadcast_to(1999 * 2000 + np.arange(2000), g.shape))
    # ... and along the far column
    g[:] = 0
    g[:, 1999] = 50000
    d2, nearest = api.host_distance_transform(g)
    assert np.array_equal(d2, np.broadcast_to((1999 - np.arange(2000, dtype=np.int64)) ** 2, g.shape))
    assert np.array_equal(nearest, np.broadcast_to(rows * 2000 + 1999, g.shape))
    g[:] = 0
    rr, cc = rng.integers(0, 2000, 3000), rng.integers(0, 2000, 3000)
    g[rr, cc] = 50000
    d2, nearest = api.host_distance_transform(g)
    # spot check against the definition on 200 cells
    for r, c in zip(rng.integers(0, 2000, 200).tolist(), rng.integers(0, 2000, 200).tolist()):
        d = (rr - r) ** 2 + (cc - c) ** 2
        assert int(d2[r, c]) == int(d.min())
        assert int(nearest[r, c]) == int((rr * 2000 + cc)[d == d.min()].min())
