"""Coarse-first window batches (csm_batch.hip: BatchGroup::coarse_first; csm_joint_kernels.hip:
k_coarse_joint_batch, k_unit_bounds): the box-max(L) level is scored first, its node keys bound the units
(pair of slices x candidate block) of the exact pass, and the exact kernel runs in two rounds on the units
whose bound can still reach the best exact key. No window here asks for a dump and every window has at
least 16 units, so the batches take that chain. Every record is compared with the oracle's literal sweep at
tolerance 0 (x, y, theta, f64 score) and with a CSM_TUNE_NO_BOUND_PASS context on the same inputs. Records
flagged EDGE_BAND or KEY_TIE are finished by the single-window path, as in test_gpu_headline.py; the seeds
are picked so that the closed form shows one candidate with the winner's key.

Small 96 x 96 maps; the windows are +-4 x +-4 candidates (one candidate block), +-4 x +-41 (12 x 84: two row
blocks of one R = 6 launch) and +-41 x +-41 (84 x 84: the R = 8 and the R = 6 launch of the exact kernel),
padded to multiples of L = 2, 4, 5."""
import math

import numpy as np
import pytest

from csm_hip import _lib as L, api, synth

import unit_bound_cases as U
from window_batch_harness import THR, Batch, _both_contexts, _context, _match_batches, _want

pytestmark = pytest.mark.gpu

CBX, CBY = 84, 48           # the fine plan's candidate block: up to 84 columns; rows: see SHAPES (one block here otherwise)
RT_SMALL = math.radians(80)
RT_TALL = math.radians(80)


def _small(seed):
    """+-4 x +-4 windows: a scan of the room's middle"""
    return synth.csm_case(seed, rows=96, cols=96, n_beams=360, max_range=1.2, init_error=(0.06, -0.04, 0.05))


def _tall(seed):
    """+-4 x +-41 windows: the sensor sits high in the map, so that no candidate offset brings a beam into the
    negative edge band (rows below 0); offsets past the high edge read unknown, which voids nothing"""
    return synth.csm_case(seed, rows=96, cols=96, n_beams=360, max_range=1.0, init_error=(0.06, -0.04, 0.05),
                          truth=(0.05, 1.3, 0.2))


def _square(seed):
    """+-41 x +-41 windows: the sensor high in both axes, for the same reason"""
    return synth.csm_case(seed, rows=96, cols=96, n_beams=360, max_range=1.0, init_error=(0.06, -0.04, 0.05),
                          truth=(1.3, 1.3, 0.2))


# the last column: candidate rows per block of the fine plan (plan_pass_pairs). 12 columns wide, R = 6 rows per lane
# cost least: 84 rows in two blocks of 42, 85 in 48 + 37; 84 columns wide it is R = 8, 48 rows, and the last 36 rows
# are the R = 6 launch of their own (tail_split): the two launches of the exact kernel
SHAPES = [
    pytest.param(_small, (21, 25), 0.4, 0.4, RT_SMALL, 2, 48, id="9x9_L2"),
    pytest.param(_small, (21, 25), 0.4, 0.4, RT_SMALL, 4, 48, id="9x9_L4"),
    pytest.param(_small, (21, 25), 0.4, 0.4, RT_SMALL, 5, 48, id="9x9_L5"),
    pytest.param(_small, (21, 25), 0.4, 0.4, math.radians(70), 4, 48, id="9x9_L4_16_units"),      # the fewest units that take the chain
    pytest.param(_tall, (21, 23), 0.4, 4.1, RT_TALL, 4, 42, id="9x83_L4"),
    pytest.param(_tall, (21, 23), 0.4, 4.1, RT_TALL, 5, 48, id="9x83_L5"),
    pytest.param(_tall, (21, 23), 0.4, 4.1, RT_TALL, 2, 42, id="9x83_L2"),
    pytest.param(_square, (21, 23), 4.1, 4.1, math.radians(60), 4, 48, id="83x83_L4_two_launches"),
]


@pytest.mark.parametrize("make,seeds,rx,ry,rt,Lr,cby", SHAPES)
def test_shapes_three_copies_and_two_maps(oracle, make, seeds, rx, ry, rt, Lr, cby):
    """Three copies of one window, then a batch that mixes two maps: the oracle's records, the same records
    without the bound pass, and units skipped."""
    cases = [make(s) for s in seeds]
    sels = [U.select_rounds(c, oracle, rx, ry, rt, Lr, CBX, cby) for c in cases]
    for sel in sels:
        assert sel["band"] == 0 and sel["ties"] == 1
        assert sel["n_theta"] % 2 == 1 and sel["units"] >= 16            # the coarse-first chain is taken
        assert sel["units"] == 16 or rt != math.radians(70)
        assert sel["round1"] + sel["round2"] < sel["units"]              # and the bounds leave units out
    want = [_want(oracle, c, rx, ry, rt, Lr) for c in cases]
    grids = {700: cases[0]["grid"], 701: cases[1]["grid"]}
    for items, expect in (([(700, cases[0])] * 3, [want[0]] * 3),
                          ([(700, cases[0]), (701, cases[1]), (701, cases[1]), (700, cases[0])],
                           [want[0], want[1], want[1], want[0]])):
        (got, flagged, (scored, skipped)), (plain, _, off_stats) = _both_contexts(items, rx, ry, rt, Lr, grids)
        assert got == expect
        assert plain == expect
        assert flagged <= len(items) // 8
        assert skipped > 0 and scored > 0, (scored, skipped)
        assert off_stats == (0, 0)
        # the units scored are the two rounds' of the restatement: the bounds are the level's, not fp32 keys
        # of the candidates (which leave fewer units), also in a window of exactly 16 units
        by_map = {700: sels[0], 701: sels[1]}
        assert scored == sum(by_map[m]["round1"] + by_map[m]["round2"] for m, _ in items)
        assert scored + skipped == sum(by_map[m]["units"] for m, _ in items)


def test_winner_outside_the_top_bound_unit(oracle):
    """A room of low values under isolated 65535 cells: the level spreads every isolated cell over L x L
    nodes, the greatest bound lies in a pair of slices that holds no good candidate, and round 1 scores
    that unit only. Round 2 must reach the winner's unit."""
    rx, ry, rt, Lr = 0.4, 0.4, RT_SMALL, 4
    cases = []
    for seed in (31, 33):
        c = _small(seed)
        rng = np.random.RandomState(seed)
        g = np.minimum(c["grid"], 9000).astype(np.uint16)
        g[rng.rand(*g.shape) < 0.02] = 65535
        g[:8, :] = 0
        g[:, :8] = 0
        c["grid"] = g
        sel = U.select_rounds(c, oracle, rx, ry, rt, Lr, CBX, CBY)
        assert sel["band"] == 0 and sel["ties"] == 1 and sel["units"] >= 16
        assert tuple(sel["top_unit"]) != tuple(sel["winner_unit"])
        assert sel["round1"] >= 1 and sel["round1_key"] < sel["best_key"]      # round 1 does not see the winner
        cases.append(c)
    items = [(710, cases[0]), (711, cases[1]), (710, cases[0])]
    want = [_want(oracle, c, rx, ry, rt, Lr) for _, c in items]
    (got, flagged, (scored, _)), (plain, _, _) = _both_contexts(items, rx, ry, rt, Lr,
                                                                 {710: cases[0]["grid"], 711: cases[1]["grid"]})
    assert got == want and plain == want
    assert flagged == 0 and scored > len(items)          # more than the one unit per window of round 1


def test_thresholded_batch_round_two_decides(oracle):
    """The coarse node's known count decides eligibility. In one of the queries the unit of the greatest bound
    does not hold the winner, so the record after round 1 is not the final one; the last query starts too far
    off and nothing in its window reaches the score threshold."""
    rx, ry, rt, Lr = 0.4, 0.4, math.radians(60), 4
    cases, behind = [], 0
    for seed in [50, 51, 52, 53, 54, 55]:
        init_error = (0.03, -0.02, 0.03) if seed != 55 else (0.3, 0.3, 0.5)
        case = synth.csm_case(seed, rows=96, cols=96, n_beams=360, max_range=1.6, init_error=init_error)
        sel = U.select_rounds(case, oracle, rx, ry, rt, Lr, CBX, CBY, *THR)
        assert sel["band"] == 0 and sel["units"] >= 16
        behind += sel["round1_key"] < sel["best_key"]
        cases.append(case)
    assert behind >= 1
    (scored, skipped), found = _match_batches(oracle, cases, rx, ry, rt, Lr, 720)
    assert skipped > 0 and scored > 0
    assert 0 < sum(found) < len(cases)            # both outcomes occur


def _nothing_eligible_case(seed, n_bright, rx, ry, rt, Lr):
    """A map of low known values; around the cells the first slice's beams end in, patches as wide as the
    window plus a node: 65535 for the first n_bright beams by angle (fewer than the known-rate threshold
    asks for), unknown for the rest. Nodes near that pose see n_bright beams on 65535 and the others on
    nothing: the greatest keys of the window, on known counts that fail the test."""
    c = synth.csm_case(seed, rows=96, cols=96, n_beams=360, max_range=1.6, init_error=(0.03, -0.02, 0.03))
    w = U.window_of(c, rx, ry, rt, Lr)
    g = np.full((96, 96), 9000, np.uint16)
    m = w["wx"] + Lr + 2
    order = np.argsort(c["angles"])
    for beams, value in ((order[:n_bright], 65535), (order[n_bright:], 0)):
        for i in beams:
            r, col = int(w["row"][0][i]), int(w["col"][0][i])
            g[max(0, r - m):r + m + 1, max(0, col - m):col + m + 1] = value
    c["grid"] = g
    return c


def test_nothing_eligible_in_round_one(oracle):
    """Every unit round 1 lists holds only nodes whose known count fails the known-rate test: the record
    after round 1 has key 0, round 2 lists every unscored unit above the score threshold's key, and the
    summary equals the oracle's (nothing found: the rest of the map is known but low)."""
    rx, ry, rt, Lr = 0.4, 0.4, math.radians(60), 4
    case = _nothing_eligible_case(51, 212, rx, ry, rt, Lr)
    assert 212 < api.host_min_known(len(case["angles"]), THR[1])
    sel = U.select_rounds(case, oracle, rx, ry, rt, Lr, CBX, CBY, *THR)
    assert sel["band"] == 0 and sel["units"] >= 16
    assert sel["round1"] >= 1 and sel["round1_key"] == 0       # units listed, nothing eligible in them
    assert sel["round2"] >= 1                                   # and round 2 has units of its own to list
    other = synth.csm_case(52, rows=96, cols=96, n_beams=360, max_range=1.6, init_error=(0.03, -0.02, 0.03))
    (scored, skipped), found = _match_batches(oracle, [case, other, case], rx, ry, rt, Lr, 750)
    sel2 = U.select_rounds(other, oracle, rx, ry, rt, Lr, CBX, CBY, *THR)
    assert found == [0, 1, 0]
    assert scored == 2 * (sel["round1"] + sel["round2"]) + sel2["round1"] + sel2["round2"]
    assert scored + skipped == 2 * sel["units"] + sel2["units"]


def _edge_case(max_range=1.2):
    """The initial pose near the map's low edges, known cells up to the edges: a box that starts in the
    negative edge band reaches the map's first known row / column (a band over unknown cells voids nothing,
    and the library knows)."""
    case = synth.csm_case(61, rows=96, cols=96, n_beams=360, max_range=max_range, init_error=(0.06, -0.04, 0.05),
                          truth=(-1.55, -1.5, 0.3))
    case["grid"][:6, :] = 30000
    case["grid"][:, :6] = 30000
    return case


def test_edge_band_keeps_every_unit(oracle):
    """Candidate offsets bring beams into the negative edge band, where a box of the level may read unknown
    under a known maximum. The bound is void: every unit is scored, the exact kernel's check against the
    level flags the records, and the single-window path's literal sweep finishes them."""
    rx, ry, rt, Lr = 0.4, 0.4, RT_SMALL, 4
    case = _edge_case()
    sel = U.select_rounds(case, oracle, rx, ry, rt, Lr, CBX, CBY)
    assert sel["band"] == 1 and sel["units"] >= 16
    assert sel["round1"] + sel["round2"] < sel["units"]          # the bounds, were they taken, would leave units out
    assert U.bound_breaks(case, oracle, rx, ry, rt, Lr) > 0      # and candidates do exceed their nodes
    items = [(730, case)] * 3
    (got, flagged, (scored, skipped)), (plain, plain_flagged, _) = _both_contexts(items, rx, ry, rt, Lr, {730: case["grid"]})
    assert skipped == 0 and scored == 3 * sel["units"]
    assert flagged == 3 and plain_flagged == 3
    assert got == [_want(oracle, case, rx, ry, rt, Lr)] * 3 and plain == got


def test_edge_band_keeps_every_unit_under_a_known_rate_threshold(oracle):
    """The same with thresholds: the fine job reads its eligibility level on every call, so
    k_bound_select's rule for the band does not apply, and only the void bound of k_unit_bounds keeps the
    units (here every bound lies below the score threshold's key: taken as bounds, they would drop all)."""
    rx, ry, rt, Lr = 0.4, 0.4, RT_SMALL, 4
    case = _edge_case()
    sel = U.select_rounds(case, oracle, rx, ry, rt, Lr, CBX, CBY, *THR)
    assert sel["band"] == 1 and sel["units"] >= 16
    assert sel["round1"] + sel["round2"] < sel["units"]
    assert U.bound_breaks(case, oracle, rx, ry, rt, Lr) > 0
    (scored, skipped), _ = _match_batches(oracle, [case], rx, ry, rt, Lr, 760)
    assert skipped == 0 and scored == sel["units"]


def test_call_to_call_and_after_a_map_update(oracle):
    """The same prepared batch scored twice, then the map changes under it (csm_update_map_with_scan), the
    level is rebuilt and new windows are scored: the oracle's records every time -- no accumulator, bound
    or level of an earlier call survives -- and the records of a context without the bound pass."""
    rx, ry, rt, Lr = 0.4, 0.4, RT_SMALL, 4
    case = _small(21)
    geom = case["geom"]
    want = [_want(oracle, case, rx, ry, rt, Lr)] * 3
    outs = {}
    for off in (0, L.TUNE_NO_BOUND_PASS):
        ctx = _context(off)
        ctx.upload_grid(740, case["grid"])
        ctx.build_pyramid(740, [1, Lr])
        batch = Batch(ctx, [(740, case)] * 3, rx, ry, rt, Lr)
        first = batch.score()
        second = batch.score()
        assert first[0] == want and second[0] == want
        assert first[1] == 0 and second[1] == 0              # one candidate holds the winner's key, no band
        assert first[2] == second[2] and (first[2][1] > 0) == (off == 0)
        shape = dict(res=geom[0], off_x=geom[1], off_y=geom[2], rows=96, cols=96, log2_block=4)
        other = _small(25)
        node = dict(pose=other["truth"], angles=other["angles"], ranges=other["ranges"], rel_pose=(0.0, 0.0, 0.0),
                    min_range=0.05, max_range=1.2)
        new_shape, _ = ctx.update_map_with_scan(740, shape, (0.0, 0.0, 0.0), node)
        grid2 = ctx.download_level(740, 0)
        assert grid2.shape != case["grid"].shape or not np.array_equal(grid2, case["grid"])
        ctx.build_pyramid(740, [1, Lr])
        case2 = dict(case, grid=grid2, geom=(new_shape["res"], new_shape["off_x"], new_shape["off_y"]))
        sel = U.select_rounds(case2, oracle, rx, ry, rt, Lr, CBX, CBY)
        third, flagged, stats = Batch(ctx, [(740, case2)] * 3, rx, ry, rt, Lr).score()
        ctx.close()
        assert third == [_want(oracle, case2, rx, ry, rt, Lr)] * 3
        clean = sel["band"] == 0 and sel["ties"] == 1
        assert flagged == 0 if clean else flagged in (0, 3)
        if off == 0 and clean:
            assert stats[0] == 3 * (sel["round1"] + sel["round2"])
        outs[off] = (first[0], third, np.array(grid2))
    assert outs[0][0] == outs[L.TUNE_NO_BOUND_PASS][0] and outs[0][1] == outs[L.TUNE_NO_BOUND_PASS][1]
    assert np.array_equal(outs[0][2], outs[L.TUNE_NO_BOUND_PASS][2])
