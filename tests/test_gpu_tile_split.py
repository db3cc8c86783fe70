"""The tile-split path of a single window: a window that gives fewer than 384 fine workgroups is
scored by a fine launch over blockIdx.z slices of the tile list, which add their partial sums
atomically, and an arg-max pass (k_argmax) over the complete sums, which also clears them for
the next query. Every window here runs on the default context and on one with
CSM_TUNE_NO_TILE_SPLIT: records, S, K and coarse K must be equal between the two and equal to
the CPU oracle's. The map is random cells with unknown blocks, so a candidate read from the
wrong accumulator word changes a sum.

The extents are the smallest that give each launch shape, worked out from plan_pass_pairs
(csm_plan.hip); blocks = candidate blocks x n_theta, slices = min(4, 492 / blocks):

  name        L  nx x ny   n_theta  plan (R, cbx x cby, ncbx x ncby)   blocks  slices
  own_known   1    7 x 7      3     6,   7 x 12, 1 x 1                    3      4
  eligible    4   12 x 12     3     6,  12 x 12, 1 x 1                    3      4
  nx_partial  1  119 x 7      3     6,  60 x 12, 2 x 1 (last: 59 wide)    6      4
  ny_partial  1    5 x 57     3     6,   5 x 30, 1 x 2 (last: 27 rows)    6      4
  r8          4    8 x 56     3     8,   8 x 56, 1 x 1                    3      4
  r8_tail     4   84 x 84     3     8,  84 x 48, 1 x 2 (last: 36 rows)    6      4
  slices_3    1    5 x 57    63     as ny_partial                       126      3
  slices_2    1    5 x 57    83     as ny_partial                       166      2
"""
import math

import numpy as np
import pytest

from csm_hip import _lib as Lb, api, synth

pytestmark = pytest.mark.gpu

MAP_ID = 41
#        name          L  wx  wy  wt  known-rate threshold
CASES = [("own_known", 1, 3, 3, 1, 0.7),
         ("eligible", 4, 5, 5, 1, 0.7),
         ("nx_partial", 1, 59, 3, 1, 0.0),
         ("ny_partial", 1, 2, 28, 1, 0.7),
         ("r8", 4, 2, 27, 1, 0.0),
         ("r8_tail", 4, 40, 40, 1, 0.0),
         ("slices_3", 1, 2, 28, 31, 0.0),
         ("slices_2", 1, 2, 28, 41, 0.7)]
LARGE, SMALL = CASES[5], CASES[0]


def _random_map_case():
    """A scan of the synthetic room over a map of random known values: a quarter of the cells and
    some 16 x 16 blocks are unknown."""
    case = synth.csm_case(23, n_beams=360)
    rng = np.random.RandomState(99)
    grid = rng.randint(1, 65535, size=case["grid"].shape).astype(np.uint16)
    grid[rng.rand(*grid.shape) < 0.25] = 0
    for _ in range(60):
        r, c = rng.randint(0, grid.shape[0] - 16), rng.randint(0, grid.shape[1] - 16)
        grid[r:r + 16, c:c + 16] = 0
    case["grid"] = grid
    return case


def _ranges_for(case, wx, wy, wt):
    """Search ranges for which the reference's window is exactly (wx, wy, wt) steps."""
    sx, sy, st = api.host_search_step(case["geom"][0], case["ranges"])
    rx, ry, rt = (2 * wx - 0.5) * sx, (2 * wy - 0.5) * sy, (2 * wt - 0.5) * st
    assert (api.host_window(rx, sx), api.host_window(ry, sy), api.host_window(rt, st)) == (wx, wy, wt)
    return rx, ry, rt, st


class _Setup:
    def __init__(self):
        self.case = _random_map_case()
        self.split = api.Context(0)
        self.whole = api.Context(0, tuning_off=Lb.TUNE_NO_TILE_SPLIT)
        levels = sorted({1} | {c[1] for c in CASES})
        for ctx in (self.split, self.whole):
            ctx.upload_grid(MAP_ID, self.case["grid"])
            ctx.build_pyramid(MAP_ID, levels)
        self.level_of = {L: i for i, L in enumerate(levels)}

    def window(self, ctx, spec):
        """(csm_window, hit columns, hit rows, search ranges) of a case."""
        _, L, wx, wy, wt, known_thr = spec
        case = self.case
        rx, ry, rt, st = _ranges_for(case, wx, wy, wt)
        sensor = api.host_compound(case["init_pose"], case["rel_pose"])
        col, row = api.host_project(case["geom"], sensor, st, wt, case["angles"], case["ranges"])
        n = len(case["angles"])
        w = ctx.make_window(2 * wt + 1, n, wx, wy, L, self.level_of[L], api.host_min_known(n, known_thr), 0.0)
        return w, col, row, (rx, ry, rt)

    def close(self):
        self.split.close()
        self.whole.close()


@pytest.fixture(scope="module")
def setup():
    s = _Setup()
    yield s
    s.close()


@pytest.mark.parametrize("spec", CASES, ids=[c[0] for c in CASES])
def test_split_equals_whole_equals_oracle(setup, oracle, spec):
    _, L, wx, wy, wt, known_thr = spec
    got = []
    for ctx in (setup.split, setup.whole):
        w, col, row, (rx, ry, rt) = setup.window(ctx, spec)
        got.append(ctx.score_window(MAP_ID, w, col, row, dump=True))
    (res, S, K, CK), (res_w, S_w, K_w, CK_w) = got
    assert res == res_w, (res, res_w)                         # every field of the csm_result record
    assert np.array_equal(S, S_w) and np.array_equal(K, K_w) and np.array_equal(CK, CK_w)
    want, oS, oK, oCK = oracle.csm_closed_form(setup.case, rx, ry, rt, L, 0.0, known_thr, dump=True)
    assert S.shape == oS.shape == (2 * wt + 1, -(-(2 * wx + 1) // L) * L, -(-(2 * wy + 1) // L) * L)
    assert np.array_equal(S, oS)
    assert np.array_equal(K, oK)
    if L > 1:
        assert np.array_equal(CK, oCK)
    assert 0 < int(K.min()) < int(K.max())                    # unknown cells under some candidates, not all
    lit = oracle.csm(setup.case, rx, ry, rt, L, 0.0, known_thr)
    assert (res["best_x"], res["best_y"], res["best_theta"]) == (lit["bestX"], lit["bestY"], lit["bestT"])
    assert res["found"] == lit["found"] == 1
    assert res["score"] == lit["scoreMax"]                    # bit-exact f64


def test_the_split_path_ran(setup):
    """One more call per case with kernel timing on: the default context launches the arg-max
    pass once per window, the CSM_TUNE_NO_TILE_SPLIT context never."""
    for ctx in (setup.split, setup.whole):
        ctx.enable_kernel_timing(True)
        ctx.reset_kernel_timing()
        for spec in CASES:
            w, col, row, _ = setup.window(ctx, spec)
            ctx.score_window(MAP_ID, w, col, row)
    ms, n = setup.split.kernel_time("argmax")
    ms_w, n_w = setup.whole.kernel_time("argmax")
    n_fine = setup.whole.kernel_time("score_fine")[1]
    for ctx in (setup.split, setup.whole):
        ctx.enable_kernel_timing(False)
    assert ms > 0 and n == len(CASES)
    assert ms_w == 0 and n_w == 0 and n_fine == len(CASES)


def test_accumulators_are_left_clean_between_windows(setup):
    """Large, small, large on ONE context: the arg-max pass of a window must leave every word it
    summed into at zero, or the next window's sums start from what was left."""
    want = {}
    for spec in (LARGE, SMALL):
        w, col, row, _ = setup.window(setup.whole, spec)
        want[spec[0]] = setup.whole.score_window(MAP_ID, w, col, row, dump=True)
    for spec in (LARGE, SMALL, LARGE, SMALL):
        w, col, row, _ = setup.window(setup.split, spec)
        res, S, K, CK = setup.split.score_window(MAP_ID, w, col, row, dump=True)
        res_w, S_w, K_w, CK_w = want[spec[0]]
        assert res == res_w, (spec[0], res, res_w)
        assert np.array_equal(S, S_w) and np.array_equal(K, K_w) and np.array_equal(CK, CK_w), spec[0]


def test_split_window_as_replayed_graph(setup):
    """csm_correlative_match records a launch shape's chain as a graph on its third query and
    replays it from the fourth on: the fine launch, the arg-max pass and its clearing."""
    _, L, wx, wy, wt, _ = CASES[1]
    case = setup.case
    rx, ry, rt, _ = _ranges_for(case, wx, wy, wt)
    timing = ("input_setup_us", "optimization_us")

    def match(ctx):
        out = ctx.correlative_match(MAP_ID, case["geom"], case["angles"], case["ranges"], case["rel_pose"],
                                    case["init_pose"], rx, ry, rt, L, 0.0, 0.0)
        return {k: v for k, v in out.items() if k not in timing}
    want = match(setup.whole)
    assert (want["win_x"], want["win_y"], want["win_theta"]) == (wx, wy, wt)
    replayed = []
    for _ in range(5):
        assert match(setup.split) == want
        replayed.append(setup.split.last_search_info()["graph_replayed"])
    assert replayed == [0, 0, 0, 1, 1], replayed
