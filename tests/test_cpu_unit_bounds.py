"""What the pruning of a coarse-first window batch rests on, without a GPU: the bound of a unit of the
exact pass (slice, candidate block) -- the greatest key of the box-max(L) nodes whose L x L candidates
intersect the block -- is at least the unit's greatest fine key. The numpy restatement
(unit_bound_cases.py) is set against the fine keys of the oracle's closed form; a node aligned one
candidate off, a block edge rounded the wrong way or an extended domain cut at 2 win + 1 shows as a
unit whose bound lies below a candidate of its own. All cases are clear of the negative edge band
(asserted): there the level bounds nothing."""
import math

import numpy as np
import pytest

from csm_hip import synth

import unit_bound_cases as U

# (seed, range x, range y, range theta, L, block columns, block rows): blocks as the fine plan cuts them
# (84 x 48 for the headline window: row blocks of 48 and 36), and blocks that are no multiple of L, so that
# nodes straddle two blocks
CASES = [
    pytest.param(3, 0.4, 0.4, math.radians(4), 2, 84, 48, id="L2_one_block"),
    pytest.param(4, 0.4, 0.4, math.radians(4), 4, 84, 48, id="L4_9_to_12"),            # 2 win + 1 = 9 -> 12
    pytest.param(5, 0.4, 0.4, math.radians(5), 5, 84, 48, id="L5_9_to_10"),
    pytest.param(6, 0.5, 0.5, math.radians(4), 5, 7, 6, id="L5_blocks_7x6"),           # 11 -> 15, straddling nodes
    pytest.param(7, 0.5, 4.1, math.radians(3), 4, 84, 48, id="L4_12x84_two_row_blocks"),
    pytest.param(8, 0.5, 4.1, math.radians(3), 2, 84, 48, id="L2_12x84"),
    pytest.param(7, 0.5, 4.1, math.radians(3), 4, 84, 42, id="L4_12x84_row_blocks_of_42"),   # what the planner cuts a 12-column window into
    pytest.param(9, 0.6, 0.6, math.radians(4), 4, 5, 9, id="L4_blocks_5x9"),
]


@pytest.mark.parametrize("seed,rx,ry,rt,L,cbx,cby", CASES)
def test_unit_bound_covers_every_candidate(oracle, seed, rx, ry, rt, L, cbx, cby):
    case = synth.csm_case(seed, rows=192, cols=192, n_beams=180, max_range=3.0)
    w = U.window_of(case, rx, ry, rt, L)
    d, fS, fK, CK = oracle.csm_closed_form(case, rx, ry, rt, L, dump=True)
    assert d["touchesBand"] == 0
    assert fS.shape == (2 * w["wt"] + 1, w["nx"], w["ny"])
    assert w["nx"] % L == 0 and w["ny"] % L == 0 and w["nx"] >= 2 * w["wx"] + 1      # the extended domain
    S, K = U.node_sums(oracle.boxmax(case["grid"], L), w)
    assert np.array_equal(K.astype(np.uint16), CK)            # the restated nodes are the oracle's nodes
    node_keys, fine_keys = U.keys_of(S, K), U.keys_of(fS, fK)
    # node <-> children, candidate by candidate
    parents = np.repeat(np.repeat(node_keys, L, axis=1), L, axis=2)
    assert np.all(parents >= fine_keys)
    # unit by unit, per slice and per pair of slices (a last single slice where n_theta is odd)
    bound, best = U.unit_bounds(node_keys, w, cbx, cby), U.unit_maxima(fine_keys, w, cbx, cby)
    assert bound.shape == (fS.shape[0], -(-w["ny"] // cby), -(-w["nx"] // cbx))
    assert np.all(bound >= best)
    assert np.all(U.pair_max(bound) >= U.pair_max(best))
    assert U.pair_max(bound).shape[0] == (fS.shape[0] + 1) // 2
    # an even number of slices (the library's windows hold 2 win_theta + 1): no single slice at the end
    assert np.all(U.pair_max(bound[:-1]) >= U.pair_max(best[:-1])) and U.pair_max(bound[:-1]).shape[0] == fS.shape[0] // 2
    # and the bound is attained by a node: it is no looser than the level itself
    assert bound.max() == node_keys.max()


def test_cases_cover_odd_and_even_slice_pairs_and_both_row_blocks(oracle):
    """The shapes above include a window with an odd and one with an even number of slice pairs, and the
    12 x 84 window has two row blocks (48 + 36 rows)."""
    pairs, row_blocks = set(), set()
    for p in CASES:
        seed, rx, ry, rt, L, cbx, cby = p.values
        w = U.window_of(synth.csm_case(seed, rows=192, cols=192, n_beams=180, max_range=3.0), rx, ry, rt, L)
        n_theta = 2 * w["wt"] + 1
        assert n_theta % 2 == 1                                # a last single slice in every window
        pairs.add(((n_theta + 1) // 2) % 2)
        row_blocks.add(len(U.blocks_of(w["ny"], cby)))
        if p.id == "L4_12x84_two_row_blocks":
            assert (w["nx"], w["ny"]) == (12, 84) and U.blocks_of(84, 48) == [(0, 48), (48, 84)]
    assert pairs == {0, 1} and {1, 2} <= row_blocks
