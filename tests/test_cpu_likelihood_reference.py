"""CPU suite: the host restatements of the likelihood field (csm_host_likelihood_kernel,
csm_host_likelihood_radius, csm_host_likelihood_map) against tests/likelihood_reference.py, equal byte for
byte; the properties the definition promises; every refusal. No GPU."""
import ctypes as C

import numpy as np
import pytest

import likelihood_reference as LR
from csm_hip import _lib as Lb, api


@pytest.mark.parametrize("sigma,res,R", [(0.05, 0.05, 3), (0.05, 0.05, 1), (0.25, 0.05, 16), (0.1, 0.05, 6),
                                         (0.03, 0.1, 2), (0.0123, 0.05, 5), (2.0, 0.05, 16), (0.001, 0.05, 4)])
def test_kernel_table_equals_the_python_table(sigma, res, R):
    got = api.host_likelihood_kernel(sigma, res, R)
    want = LR.kernel(sigma, res, R)
    assert got.dtype == np.uint32 and got.tolist() == want.tolist()
    assert got[0] == 32768
    assert (np.diff(got.astype(np.int64)) <= 0).all()


def test_radius_and_its_clamps():
    for sigma, res in [(0.05, 0.05), (0.25, 0.05), (0.1, 0.05), (0.0001, 0.05), (5.0, 0.05), (0.08, 0.05),
                       (0.26666, 0.05), (0.2667, 0.05), (1e-300, 1.0), (1e300, 1e-300)]:
        assert api.host_likelihood_radius(sigma, res) == LR.radius(sigma, res), (sigma, res)
    assert api.host_likelihood_radius(0.05, 0.05) == 3
    assert api.host_likelihood_radius(0.0001, 0.05) == 1             # clamped from below
    assert api.host_likelihood_radius(5.0, 0.05) == 16               # ... and from above
    assert api.host_likelihood_radius(0.25, 0.05) == 15


@pytest.mark.parametrize("keep_unknown", [False, True])
@pytest.mark.parametrize("name,R", LR.CPU_CASES)
def test_host_map_equals_the_reference(name, R, keep_unknown):
    g, t, want = LR.expected(name, R, keep_unknown)
    occ = LR.occupied_min_of(name)
    got = api.host_likelihood_map(g, radius=R, occupied_min=occ, keep_unknown=keep_unknown, kernel=t)
    assert got.dtype == np.uint16 and got.shape == g.shape
    assert np.array_equal(got, want)
    assert int(got.max(initial=0)) <= 65534
    far = LR.far_from_obstacles(g, R, occ)
    assert np.array_equal(got[far], g[far])                          # no obstacle within R: unchanged
    assert (got >= g).all()
    if keep_unknown:
        assert not got[g == 0].any()
    assert int(got.max(initial=0)) == int(g.max(initial=0))           # T <= 32768: nothing above the largest value


def test_the_cases_cover_what_they_claim():
    g, _, out = LR.expected("csm_case0", 3, False)
    changed = out != g
    assert changed.sum() > 3000 and (changed & (g == 0)).sum() > 1000    # a do-nothing build cannot pass
    _, _, kept = LR.expected("csm_case0", 3, True)
    assert (kept != out).sum() > 1000                                    # ... nor one that ignores keep_unknown
    g, _, out = LR.expected("threshold", 3, False)
    assert out[4, 5] > g[4, 5] and out[4, 31] == g[4, 31] and out[19, 6] > 0
    assert LR.expected("threshold", 3, True)[2][19, 6] == 0
    g, _, out = LR.expected("extremes", 3, False)
    assert out[15, 16] > 1 and out[3, 4] == 1 and out[15, 15] == 65534
    assert not LR.expected("all_unknown", 3, False)[2].any()
    g, _, out = LR.expected("all_obstacle", 3, False)
    assert np.array_equal(out, g)
    g, _, out = LR.expected("corners", 16, False)
    assert out[1, 1] > 0 and out[-2, -2] > 0 and out[1, -2] > 0 and out[-2, 1] > 0
    for name, _ in LR.CPU_CASES + LR.GPU_EXTRA_CASES:
        assert int(LR.grid_of(name).max(initial=0)) <= 65534


def _id(case):
    return "%s-R%d-%s-%d" % case


@pytest.mark.parametrize("keep_unknown", [False, True])
@pytest.mark.parametrize("case", LR.EDGE_CASES, ids=_id)
def test_host_map_equals_the_reference_at_the_edge_cases(case, keep_unknown):
    name, R, kind, occ = case
    g, t, want = LR.edge_expected(name, R, kind, occ, keep_unknown)
    got = api.host_likelihood_map(g, radius=R, occupied_min=occ, keep_unknown=keep_unknown, kernel=t)
    assert got.dtype == np.uint16 and got.shape == g.shape
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    far = LR.far_from_obstacles(g, R, occ)
    assert np.array_equal(got[far], g[far])                          # no obstacle within R: unchanged
    assert (got >= g).all()
    if keep_unknown:
        assert not got[g == 0].any()
    assert int(got.max(initial=0)) == int(g.max(initial=0))           # T <= 32768: nothing above the largest value
    if name == "single_65535":
        assert int(got.max()) == 65535 and got[LR.SINGLE_AT] == 65535   # the largest value survives unwrapped
    else:
        assert int(got.max(initial=0)) <= 65534


def test_first_known_and_halo_counts_on_hand_made_grids():
    g = np.zeros((70, 140), np.uint16)
    assert LR.first_known(g) == (70, 140)
    g[40, 9] = 1
    g[13, 77] = 65535
    assert LR.first_known(g) == (13, 9)
    g[31, 63] = g[32, 64] = g[69, 139] = 40000
    g[28, 60] = 32767                                                 # not an obstacle
    # tiles: rows 0..31 / 32..63 / 64..69, columns 0..63 / 64..127 / 128..139
    assert LR.halo_counts(g, 1).tolist() == [[2, 3, 0], [2, 2, 0], [0, 0, 1]]
    assert LR.halo_counts(g, 16).tolist() == [[3, 3, 0], [2, 3, 1], [0, 1, 1]]
    assert LR.halo_counts(g, 1, 1).tolist() == [[3, 3, 0], [3, 2, 0], [0, 0, 1]]


def test_the_edge_cases_are_what_they_claim():
    # the tables
    for R in (1, 3, 16):
        ramp = LR.table_of("ramp", R).tolist()
        assert ramp[0] == 32768 and len(set(ramp)) == len(ramp) == R * R + 1 and max(ramp) <= 32768
        assert set(LR.table_of("flat", R).tolist()) == {32768} and not LR.table_of("zero", R).any()
    # the switch: exactly (2R + 1)^2 obstacles in the one tile's halo, and one more
    for R, n in ((1, 9), (3, 49), (16, 1089)):
        assert LR.switch_count(R) == n
        assert LR.halo_counts(LR.grid_of("switch_%d" % R), R).tolist() == [[n]]
        assert LR.halo_counts(LR.grid_of("switch_%d_plus" % R), R).tolist() == [[n + 1]]
    assert LR.halo_counts(LR.grid_of("switch_two_tiles"), 3).tolist() == [[50, 49]]
    # one over at R = 16 with the obstacles of the last rows each alone responsible for a cell: without any
    # one of the last 44 the reference changes under it
    g, t, out = LR.edge_expected("switch_16_last", 16, "ramp", 32768, True)
    assert LR.halo_counts(g, 16).tolist() == [[1090]] and int((g[16:] >= 32768).sum()) == 110
    under = 1 + ((65533 * int(t[1])) >> 15)
    for r in LR.LAST_ROWS:
        assert (g[r, ::3] == 65534).all() and (out[r + 1, ::3] == under).all()
    for r in LR.LAST_ROWS[-2:]:
        for c in range(0, 64, 3):
            less = g.copy()
            less[r, c] = 700
            assert LR.likelihood_map(less, t, 16, 32768, True)[r + 1, c] < under
    # dense: past the switch in all four tiles at R = 3. At R = 16 only tile (0, 0) of the 40 x 70 map can be
    # (the three others see 40 x 22, 24 x 70 and 24 x 22 cells, of which 60 % are obstacles: fewer than 1089);
    # the 60 x 100 map is past it in all four, partial tiles and 4 pad columns included.
    assert LR.halo_counts(LR.grid_of("dense40x70"), 3).shape == (2, 2)
    assert (LR.halo_counts(LR.grid_of("dense40x70"), 3) > 49).all()
    h = LR.halo_counts(LR.grid_of("dense40x70"), 16)
    assert h[0, 0] > 1089 and (h > 0).all() and (h.reshape(-1)[1:] <= 1089).all()
    assert LR.halo_counts(LR.grid_of("dense60x100"), 16).shape == (2, 2)
    assert (LR.halo_counts(LR.grid_of("dense60x100"), 16) > 1089).all()
    # the taps path's rim: past the switch in the upper tile at every radius, and around the lone obstacle
    # the flat output is the disc, rim cells included (an off-axis one for R = 5, 10, 13, 15)
    g = LR.grid_of("dense_rim")
    r0, c0 = LR.RIM_AT
    y, x = np.ogrid[:64, :64]
    d2 = (y - r0) ** 2 + (x - c0) ** 2
    alone = g.copy()
    alone[r0, c0] = 700
    for R, off in ((5, (3, 4)), (10, (6, 8)), (13, (5, 12)), (15, (9, 12)), (16, None)):
        assert LR.halo_counts(g, R)[0, 0] > LR.switch_count(R)
        out = LR.edge_expected("dense_rim", R, "flat", 32768, False)[2]
        near = (d2 <= (R + 1) ** 2) & (x < 24)
        assert LR.far_from_obstacles(alone, R)[near].all()              # no other obstacle reaches these cells
        assert np.array_equal(out[near] == 50000, (d2 <= R * R)[near]) and (out[near & (d2 > R * R)] < 32768).all()
        assert out[r0 + R, c0] == 50000 and out[r0, c0 + R] == 50000    # on the rim, inside the map
        if off:
            assert off[0] ** 2 + off[1] ** 2 == R * R and out[r0 + off[0], c0 + off[1]] == 50000
    h = LR.halo_counts(LR.grid_of("room200"), 16)                       # walls: long lists, never past the switch
    assert h.shape == (7, 4) and 300 < int(h.max()) <= 1089 and int((h > 100).sum()) >= 12
    # the flat output of one obstacle is its disc
    r0, c0 = LR.SINGLE_AT
    y, x = np.ogrid[:48, :80]
    d2 = (y - r0) ** 2 + (x - c0) ** 2
    for R in (2, 5, 10, 13, 15, 16):
        out = LR.edge_expected("single", R, "flat", 32768, False)[2]
        assert np.array_equal(out != 0, d2 <= R * R) and set(out[out != 0].tolist()) == {50000}
        assert int((out != 0).sum()) == LR.disc_cells(R)
        rim = (d2 == R * R) & (y != r0) & (x != c0)
        assert bool(rim.any()) == (R in (5, 10, 13, 15))                # an off-axis cell exactly on the rim
        ramp = LR.edge_expected("single", R, "ramp", 32768, False)[2]
        t = LR.table_of("ramp", R).astype(np.int64)
        assert np.array_equal(ramp, np.where(d2 <= R * R, 1 + ((49999 * t[np.minimum(d2, R * R)]) >> 15), 0))
        assert not LR.edge_expected("single", R, "flat", 32768, True)[2][d2 != 0].any()
    assert [LR.disc_cells(R) for R in (1, 2, 3, 5, 16)] == [5, 13, 29, 81, 797]
    zero = LR.edge_expected("single", 5, "zero", 32768, False)[2]
    assert np.array_equal(zero, np.where(d2 == 0, 50000, np.where(d2 <= 25, 1, 0)))
    # the lines and the cell
    assert LR.grid_of("line1xN").shape == (1, 200) and LR.grid_of("lineNx1").shape == (200, 1)
    assert np.flatnonzero(LR.grid_of("line1xN") >= 32768).tolist() == [0, 63, 64, 65, 199]
    assert np.flatnonzero(LR.grid_of("lineNx1") >= 32768).tolist() == [0, 31, 32, 33, 63, 64, 65, 199]
    assert LR.grid_of("one_cell").tolist() == [[50000]]
    # occupied_min: 40000 keeps some obstacles and drops others; from 65535 on the map is copied through
    g = LR.grid_of("random37x53")
    assert 0 < int((g >= 40000).sum()) < int((g >= 32768).sum())
    a, b = LR.edge_expected("random37x53", 3, "gauss", 40000, False)[2], LR.expected("random37x53", 3, False)[2]
    assert (a != b).any() and (a != g).any()
    for occ in (65535, 70000):
        assert np.array_equal(LR.edge_expected("random37x53", 3, "gauss", occ, False)[2], g)
    # low_known: the field's first known row and column lie in the band the source has none in
    g, _, spread = LR.edge_expected("low_known", 3, "gauss", 32768, False)
    assert g[9].any() and g[:, 11].any() and LR.first_known(g) == (9, 11)
    fr, fc = LR.first_known(spread)
    assert fr < 9 and fc < 11
    assert fr <= LR.LOW_KNOWN_OBSTACLE[0] - 3 and fc <= LR.LOW_KNOWN_OBSTACLE[1] - 3
    assert LR.first_known(LR.edge_expected("low_known", 3, "gauss", 32768, True)[2]) == (9, 11)
    assert LR.first_known(LR.edge_expected("all_unknown", 3, "gauss", 32768, False)[2]) == (20, 33)


def test_default_table_and_radius_come_from_sigma():
    g = LR.grid_of("random37x53")
    got = api.host_likelihood_map(g, 0.05, 0.05)
    want = LR.likelihood_map(g, LR.kernel(0.05, 0.05, 3), 3)
    assert np.array_equal(got, want)


def test_argument_errors_return_their_codes():
    lib = Lb.load()
    g = np.ascontiguousarray(LR.grid_of("random16"))
    out = np.zeros_like(g)
    table = LR.kernel(0.05, 0.05, 3)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def run(radius=3, occupied_min=32768, kernel=table, rows=16, cols=16, grid=g, dst=out):
        p = Lb.LikelihoodParams(radius, occupied_min, 0, 0, None if kernel is None else kernel.ctypes.data)
        return lib.csm_host_likelihood_map(None if grid is None else ptr(grid), rows, cols, C.byref(p),
                                           None if dst is None else ptr(dst))

    assert run() == Lb.CSM_OK
    for bad in (dict(radius=0), dict(radius=17), dict(radius=-1), dict(occupied_min=0), dict(kernel=None),
                dict(rows=0), dict(cols=0), dict(grid=None), dict(dst=None)):
        assert run(**bad) == Lb.CSM_EINVAL, bad
    over = table.copy()
    over[9] = 32769
    assert run(kernel=over) == Lb.CSM_EINVAL
    over[9] = 32768
    assert run(kernel=over) == Lb.CSM_OK
    assert lib.csm_host_likelihood_map(ptr(g), 16, 16, None, ptr(out)) == Lb.CSM_EINVAL

    t = np.zeros(300, np.uint32)
    for sigma, res, R in [(0.0, 0.05, 3), (-1.0, 0.05, 3), (0.05, 0.0, 3), (float("nan"), 0.05, 3),
                          (0.05, float("inf"), 3), (0.05, 0.05, 0), (0.05, 0.05, 17)]:
        assert lib.csm_host_likelihood_kernel(sigma, res, R, ptr(t)) == Lb.CSM_EINVAL
    assert lib.csm_host_likelihood_kernel(0.05, 0.05, 3, None) == Lb.CSM_EINVAL
    for sigma, res in [(0.0, 0.05), (0.05, 0.0), (float("nan"), 0.05), (float("inf"), 0.05), (-0.1, 0.05)]:
        assert lib.csm_host_likelihood_radius(sigma, res) == Lb.CSM_EINVAL
        with pytest.raises(api.CsmError):
            api.host_likelihood_radius(sigma, res)
