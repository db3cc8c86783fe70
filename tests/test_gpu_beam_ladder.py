"""The window chains on both sides of every beam-count threshold of the code (beam_ladder_cases.py: the
rungs, computed from the restated size rules; test_cpu_beam_ladder_cases.py: their literal values and the
premises of every case used here).

  a. the 3 x 12 x 84 window of test_gpu_pair_window.py cast at every rung, through every batch chain and
     the single-window path: S and K of EVERY candidate against the oracle's closed form, and
     bound_pass_stats() says which chain ran -- the joint / per-slice switch is pinned to 4248 | 4249;
  b. the coarse-first chain (k_coarse_joint_batch, k_unit_bounds, two rounds of the exact kernel) at 3072,
     3073, 4248 and, on per-slice lists, 4249 beams: records against the oracle's literal sweep, and the units
     scored against the numpy restatement of the level's node sums -- wrong node sums seldom move the winner,
     but they move the units the bounds keep;
  c. the same for pairs of slices with more than 8 records (the kernel reloads its record words) and with
     a tile cut into several records (more than kJRec entries);
  d. csm_correlative_match_batch with the loop detector's thresholds at 3073 and 4248 beams (the level's
     known counts, two 16-bit halves of one word, decide eligibility at about 0.6 n);
  e. scans of 360, 3073 and 4248 beams in one call, and 4248 with 4249 (the longer scan takes the group to
     per-slice lists);
  f. the near-tie landscapes of test_gpu_bound_pass.py at 4248 beams on the fp32 chain.

All comparisons are at tolerance 0, except the fp32 keys of (a), which obey the bound the bound pass
states. The harnesses are those of the files named: imported, not restated."""
import numpy as np
import pytest
import torch

from csm_hip import api

import beam_ladder_cases as B
from test_gpu_bound_pass import _run as _run_copies
from test_gpu_pair_window import BATCH_RUNS, NT, NX, NY, _batch, _make
from window_batch_harness import THR, _both_contexts, _match_batches, _want

pytestmark = pytest.mark.gpu

LADDER = B.ladder(20)                   # the pair window's frame has 20 endpoint tiles
JOINT_MAX = B.rungs(20)["joint_lists"][0][0]


# ---- a. every candidate, every chain, at every rung ----

_pair_windows = {}


def _pair_window(oracle, n, saturated):
    """The window with the closed form's S and K of every candidate, made once per (beams, grid)."""
    if (n, saturated) not in _pair_windows:
        _pair_windows[n, saturated] = _make(B.pair_window_case(n, saturated), oracle)
    return _pair_windows[n, saturated]


@pytest.mark.parametrize("saturated", [False, True], ids=["room", "saturated"])
@pytest.mark.parametrize("n", LADDER)
def test_every_candidate_every_chain(oracle, n, saturated):
    assert (NT, NX, NY) == B.PAIR_SHAPE and LADDER == [682, 683, 1365, 1366, 2730, 2731, 3072, 3073, 4248, 4249,
                                                         5461, 5462, 10240]
    w = _pair_window(oracle, n, saturated)
    if saturated:
        assert int(w["K"].max()) == n and int(w["S"].max()) == 65535 * n
    else:
        assert int(w["K"].min()) < int(w["K"].max()) and int(w["S"].max()) > 0
    joint = n <= JOINT_MAX
    for name, tuning_off in BATCH_RUNS:
        want_f32 = name == "default" and joint
        S, K, F, (scored, skipped) = _batch(w, tuning_off, want_f32=want_f32)
        for k in range(2):
            assert np.array_equal(K[k], w["K"]), (name, n, k)
            assert np.array_equal(S[k], w["S"]), (name, n, k)
        if name == "default" and joint:
            # a dump asks for every block: the exact list kernel scored all of them behind the fp32 pass
            assert scored > 0 and skipped == 0, (n, scored, skipped)
            key = 32268.0 * w["K"].astype(np.float64) + 499.0 * w["S"].astype(np.float64)
            for k in range(2):
                err = np.abs(F[k].astype(np.float64) - key)
                assert np.all(err <= (n + 3) * 2.0 ** -24 * key + 1e-9), (n, k, float(err.max()))
        else:
            # per-slice lists from JOINT_MAX + 1 beams on, and in the chains without a bound pass
            assert (scored, skipped) == (0, 0), (name, n)
    ctx = api.Context(0)
    try:
        ctx.upload_grid(1, w["case"]["grid"])
        ctx.build_pyramid(1, [1, B.PAIR_L])
        wx, wy, wt = w["win"]
        win = ctx.make_window(2 * wt + 1, n, wx, wy, B.PAIR_L, 1, api.host_min_known(n, 0.0), 0.0)
        _, S, K, _ = ctx.score_window(1, win, w["col"], w["row"], dump=True)
    finally:
        ctx.close()
    assert np.array_equal(K, w["K"]) and np.array_equal(S, w["S"])


# ---- b, c. coarse-first at the rungs; record handling of k_coarse_joint_batch ----

def _coarse_first_family(oracle, name, n):
    """Three copies of one window, then a batch mixing two maps, on a default context and on one without the
    bound pass: the oracle's records on both, nothing flagged, and the units scored / skipped that
    select_rounds restates from the level's node sums -- or (0, 0) where the scans are too long for joint lists."""
    f = B.FAMILIES[name]
    seeds = f.seeds[:2]
    cases = [f.case(s, n) for s in seeds]
    sels = [f.premises(oracle, s, n) for s in seeds]
    for sel in sels:            # asserted for every seed in test_cpu_beam_ladder_cases.py; the chain is taken
        assert sel["units"] >= 16 and sel["band"] == 0 and sel["ties"] == 1
        assert sel["round1"] + sel["round2"] < sel["units"]
    joint = B.joint_lists(sels[0]["tiles"], n)
    want = [_want(oracle, c, f.rx, f.ry, f.rt, f.Lr) for c in cases]
    grids = {800: cases[0]["grid"], 801: cases[1]["grid"]}
    by_map = {800: sels[0], 801: sels[1]}
    for items, expect in (([(800, cases[0])] * 3, [want[0]] * 3),
                          ([(800, cases[0]), (801, cases[1]), (801, cases[1]), (800, cases[0])],
                           [want[0], want[1], want[1], want[0]])):
        (got, flagged, stats), (plain, plain_flagged, off_stats) = _both_contexts(items, f.rx, f.ry, f.rt, f.Lr, grids)
        assert got == expect, (name, n)
        assert plain == expect, (name, n)
        assert flagged == 0 and plain_flagged == 0
        assert off_stats == (0, 0)
        if joint:
            scored, skipped = stats
            assert scored == sum(by_map[m]["round1"] + by_map[m]["round2"] for m, _ in items), (name, n, stats)
            assert scored + skipped == sum(by_map[m]["units"] for m, _ in items), (name, n, stats)
        else:
            assert stats == (0, 0), (name, n)
    return sels


@pytest.mark.parametrize("n", B.RUNG_BEAMS)
@pytest.mark.parametrize("name", ["rungs_small", "rungs_tall"])
def test_coarse_first_at_the_rungs(oracle, name, n):
    sels = _coarse_first_family(oracle, name, n)
    assert all(sel["lists"]["max_beams"] > B.K_MAX_MULT for sel in sels)       # beams of a cell split over entries


def test_more_than_eight_records_per_pair(oracle):
    """k_coarse_joint_batch hands out the words of 8 records at a time: with 10 records the wave loads a
    second group (rec_group(ti + 1) at (ti + 1) & 7 == 0)."""
    sels = _coarse_first_family(oracle, "many_records", 1080)
    assert all(sel["lists"]["records"] > 8 for sel in sels)


def test_tile_cut_into_several_records(oracle):
    """A noisy room scan of 4248 beams: one endpoint tile of the pair holds more than kJRec = 256 entries
    and becomes two records with one tile number, one bounding box and two pieces of the list; the bounds
    still leave units out (13 of 17 and 14 of 17 are scored)."""
    sels = _coarse_first_family(oracle, "split_tile", 4248)
    assert all(sel["lists"]["max_entries"] > B.K_JREC and sel["lists"]["max_records"] >= 2 for sel in sels)


# ---- d. thresholded batches at the rungs ----

@pytest.mark.parametrize("n", [3073, 4248])
def test_thresholded_batches_at_the_rungs(oracle, n):
    """rungs_small with one query started too far off: at 1.2 m no query reaches the score threshold
    (test_cpu_beam_ladder_cases.py: no seed does), so every summary is `not found`. The 1.6 m queries of
    test_gpu_coarse_first.py's thresholded batch at the same beam counts, with one started too far off, give
    both outcomes. Summaries against the oracle's literal sweep, the two contexts agree, and the units are
    those the restatement selects with the level's known counts deciding eligibility."""
    outcomes = []
    for near, far, first_id in (("rungs_small", "rungs_small_far", 820), ("rungs_reach", "rungs_reach_far", 830)):
        fams = [B.FAMILIES[near]] * len(B.FAMILIES[near].seeds) + [B.FAMILIES[far]]
        seeds = B.FAMILIES[near].seeds + B.FAMILIES[far].seeds[:1]
        f = fams[0]
        cases = [fam.case(s, n) for fam, s in zip(fams, seeds)]
        sels = [fam.premises(oracle, s, n, *THR) for fam, s in zip(fams, seeds)]
        assert all(sel["units"] >= 16 and sel["band"] == 0 for sel in sels)
        (scored, skipped), found = _match_batches(oracle, cases, f.rx, f.ry, f.rt, f.Lr, first_id)
        assert found == [sel["found"] for sel in sels]
        assert found[-1] == 0
        assert scored == sum(sel["round1"] + sel["round2"] for sel in sels), (near, n, scored, skipped)
        assert scored + skipped == sum(sel["units"] for sel in sels), (near, n, scored, skipped)
        outcomes += found
    assert 0 < sum(outcomes) < len(outcomes)            # both outcomes occur


# ---- e. mixed scan lengths in one call ----

def test_mixed_scan_lengths_in_one_call(oracle):
    """Windows of one shape and different beam counts are one group of the call. 360, 3073 and 4248 beams: joint
    lists with a table size per query, coarse-first units as restated. 4248 with 4249: the group's longest scan
    does not fit the joint table and all of it goes to per-slice lists, without a bound pass."""
    f = B.FAMILIES["rungs_small"]
    grids = {840: f.case(21, 360)["grid"], 841: f.case(25, 360)["grid"]}
    for picks, joint in (([(840, 21, 360), (841, 25, 3073), (840, 21, 4248), (840, 21, 360)], True),
                         ([(840, 21, 4248), (841, 25, 4249), (840, 21, 4248)], False)):
        items = [(m, f.case(s, n)) for m, s, n in picks]
        for (m, s, n), (_, case) in zip(picks, items):
            assert np.array_equal(case["grid"], grids[m]) and len(case["angles"]) == n      # the map does not depend on the beams
        sels = [f.premises(oracle, s, n) for _, s, n in picks]
        assert all(sel["units"] >= 16 and sel["band"] == 0 and sel["ties"] == 1 for sel in sels)
        assert all(B.joint_lists(sel["tiles"], n) for sel, (_, _, n) in zip(sels, picks)) == joint
        expect = [_want(oracle, c, f.rx, f.ry, f.rt, f.Lr) for _, c in items]
        (got, flagged, stats), (plain, plain_flagged, off_stats) = _both_contexts(items, f.rx, f.ry, f.rt, f.Lr, grids)
        assert got == expect and plain == expect
        assert flagged == 0 and plain_flagged == 0 and off_stats == (0, 0)
        if joint:
            assert stats[0] == sum(sel["round1"] + sel["round2"] for sel in sels), stats
            assert stats[0] + stats[1] == sum(sel["units"] for sel in sels), stats
        else:
            assert stats == (0, 0)


# ---- f. near ties at the joint limit ----

@pytest.mark.parametrize("kind", ["checker", "noise"])
def test_near_ties_at_the_joint_limit(oracle, kind):
    """8 units: the packed-fp32 bound pass decides which blocks the exact kernel scores, with
    approx_slack = 4 (n + 3) 2^-24 at the greatest n that has joint lists. Records flagged KEY_TIE are
    finished by score_window, as in test_gpu_bound_pass.py; every record equals the oracle's."""
    case = B.near_tie_case(kind)
    assert len(case["angles"]) == JOINT_MAX
    ctx = api.Context(0)
    try:
        ctx.set_stream(torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream)
        final, (scored, skipped) = _run_copies(ctx, case, B.TIE_RX, B.TIE_RY, B.TIE_RT, B.TIE_L)
    finally:
        ctx.close()
    assert all(rec == _want(oracle, case, B.TIE_RX, B.TIE_RY, B.TIE_RT, B.TIE_L) for rec in final), (kind, final[0])
    assert scored > 0 and scored + skipped == 3 * 8, (scored, skipped)       # the fp32 chain: 3 copies x 8 units
