"""GPU parity: the winner of a window under a motion prior (csm_score_window_prior,
csm_correlative_match_prior, csm_correlative_match_prior_batch) against tests/prior_reference.py. Bar: every
integer equal, every double bit-equal; nothing carries a tolerance."""
import functools
import math

import numpy as np
import pytest

import peaks_reference as PR
import prior_reference as P
from csm_hip import _lib as Lb, api, synth
from test_gpu_peaks import CASES, ELIG_RANGE, RANGE, _elig_case, _threshold_that_bites, _uniform_case, _vol_bytes

MAP = 900


def sym(xx, yy, tt, xy=0.0, xt=0.0, yt=0.0):
    return np.array([[xx, xy, xt], [xy, yy, yt], [xt, yt, tt]], np.float64)


# score units per m^2 / rad^2: a score is in [0, 1], the windows reach 0.5 m and 0.1 rad from the centre
LAMBDAS = dict(zero=sym(0.0, 0.0, 0.0),
               diag=sym(2.0, 2.0, 40.0),                        # moderate, diagonal
               full=sym(3.0, 2.0, 60.0, 1.0, 4.0, -3.0),        # positive definite, every cross term
               indef=sym(1.5, 1.5, 20.0, 2.5))                  # one negative eigenvalue: the clamp acts
assert np.linalg.eigvalsh(LAMBDAS["full"]).min() > 0 > np.linalg.eigvalsh(LAMBDAS["indef"]).min()


@functools.lru_cache(maxsize=None)
def _volume(seed, L):
    """(case, volume) of one of the six cases: computed once, shared, never changed."""
    case = synth.csm_case(seed)
    return case, P.volume(case, *RANGE, L)


@functools.lru_cache(maxsize=None)
def _six(seed, L, name):
    """(case, volume, reference, clamped candidates) of a case under LAMBDAS[name]."""
    case, vol = _volume(seed, L)
    return (case, vol) + P.prior(vol, case, LAMBDAS[name])


def _window(ctx, case, win, L, score_thr=0.0, known_thr=0.0, map_id=MAP):
    """Uploads the map and returns the csm_window of the reference's window."""
    wx, wy, wt = win["win"]
    ctx.upload_grid(map_id, case["grid"])
    ctx.build_pyramid(map_id, [1, L])
    n = len(case["angles"])
    return ctx.make_window(2 * wt + 1, n, wx, wy, L, 1 if L > 1 else 0, api.host_min_known(n, known_thr), score_thr)


def _match(ctx, case, rng, L, lam, map_id=MAP, **kw):
    return ctx.correlative_match_prior(map_id, case["geom"], case["angles"], case["ranges"], case["rel_pose"],
                                       case["init_pose"], *rng, L, lam, **kw)


def _with_band(ref, band):
    """The reference with the edge-band flag on the records that are found."""
    mark = lambda r: dict(r, flags=r["flags"] | band) if r["found"] else r
    return dict(ref, best=mark(ref["best"]), unweighted=mark(ref["unweighted"]))


def _check_summary(out, ref, win, case, band=0):
    assert out["prior"] == _with_band(ref, band)
    s = out["summary"]
    assert s["raw"] == out["prior"]["best"] and s["pose_found"] == ref["best"]["found"]
    assert (s["win_x"], s["win_y"], s["win_theta"]) == win["win"]
    assert (s["step_x"], s["step_y"], s["step_theta"]) == tuple(win["steps"])
    assert s["candidates"] == int(np.prod(win["shape"]))
    if ref["best"]["found"]:
        best, est = PR.poses_of(ref["best"], win, case["rel_pose"])
        assert s["best_sensor_pose"] == best and s["estimated_pose"] == est       # bit-exact doubles


strip = lambda o: {k: v for k, v in o.items() if not k.endswith("_us")}


@pytest.mark.gpu
@pytest.mark.parametrize("seed,L", CASES)
def test_six_cases_under_four_priors(gpu_ctx, seed, L):
    case, vol = _volume(seed, L)
    win = vol["win"]
    w = _window(gpu_ctx, case, win, L)
    args = (MAP, case["geom"], case["angles"], case["ranges"], case["rel_pose"], case["init_pose"], *RANGE, L)
    before = gpu_ctx.correlative_match(*args)
    peak0 = gpu_ctx.score_window_peaks(MAP, w, win["col"], win["row"], 1)[0]
    for name, lam in LAMBDAS.items():
        ref = _six(seed, L, name)[2]
        got = gpu_ctx.score_window_prior(MAP, w, win["col"], win["row"], lam, win["steps"])
        assert got == ref
        assert got["unweighted"] == peak0
        _check_summary(_match(gpu_ctx, case, RANGE, L, lam), ref, win, case)
    after = gpu_ctx.correlative_match(*args)
    assert strip(before) == strip(after) and after["raw"] == peak0
    gpu_ctx.release_grid(MAP)


@pytest.mark.gpu
def test_a_zero_prior_changes_nothing(gpu_ctx):
    for seed, L in CASES:
        case, vol = _volume(seed, L)
        win = vol["win"]
        w = _window(gpu_ctx, case, win, L)
        got = gpu_ctx.score_window_prior(MAP, w, win["col"], win["row"], LAMBDAS["zero"], win["steps"])
        assert got["best"] == got["unweighted"] and got["best"]["found"] == 1
        assert got["penalty"] == 0 and got["penalised_key"] == got["best"]["key"] and got["Q"] == [0] * 6
        gpu_ctx.release_grid(MAP)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 2])
def test_all_ties_map_the_prior_picks_the_centre(gpu_ctx, L):
    """More than 8192 candidates, thousands of them tied in key and f64 score over several workgroups."""
    case = _uniform_case()
    rng = (1.2, 1.2, math.radians(24))
    vol = P.volume(case, *rng, L)
    win = vol["win"]
    wx, wy, wt = win["win"]
    nt, nx, ny = win["shape"]
    assert nt * nx * ny > 8192 and vol["cf"]["touchesBand"] == 0
    w = _window(gpu_ctx, case, win, L)
    key = 32268 * vol["K"].astype(np.int64) + 499 * vol["S"].astype(np.int64)
    tied = np.argwhere(key == key.max())        # known rate threshold 0: every candidate is eligible
    rank = lambda c: ((c[0] * (nx // L) + c[1] // L) * (ny // L) + c[2] // L) * L * L + (c[1] % L) * L + c[2] % L
    first = min(tied.tolist(), key=rank)

    ref, _ = P.prior(vol, case, LAMBDAS["zero"])
    u = ref["unweighted"]
    assert u["tie_count"] == len(tied) > 1000 and u["flags"] == Lb.FLAG_KEY_TIE | Lb.FLAG_F64_TIE
    assert [u["best_theta"] + wt, u["best_x"] + wx, u["best_y"] + wy] == first    # the corner, far from the guess
    assert gpu_ctx.score_window_prior(MAP, w, win["col"], win["row"], LAMBDAS["zero"], win["steps"]) == ref

    for lam in (sym(1e-5, 1e-5, 1e-4), sym(5.0, 5.0, 100.0), sym(2.0, 0.3, 7.0)):     # any positive diagonal
        ref, _ = P.prior(vol, case, lam)
        b = ref["best"]
        assert (b["best_x"], b["best_y"], b["best_theta"]) == (0, 0, 0) and b["tie_count"] == 1 and b["flags"] == 0
        assert ref["penalty"] == 0 and ref["unweighted"] == u
        assert gpu_ctx.score_window_prior(MAP, w, win["col"], win["row"], lam, win["steps"]) == ref
        _check_summary(_match(gpu_ctx, case, rng, L, lam), ref, win, case)

    lam = sym(2.0, 0.0, 0.0)                    # positive in x only: the first in sweep order among x = 0
    ref, _ = P.prior(vol, case, lam)
    b = ref["best"]
    first_x0 = min([c for c in tied.tolist() if c[1] == wx], key=rank)
    assert [b["best_theta"] + wt, b["best_x"] + wx, b["best_y"] + wy] == first_x0 and b["best_x"] == 0
    assert 1 < b["tie_count"] == sum(c[1] == wx for c in tied.tolist()) < u["tie_count"]
    assert b["flags"] == Lb.FLAG_KEY_TIE | Lb.FLAG_F64_TIE and ref["penalty"] == 0
    assert gpu_ctx.score_window_prior(MAP, w, win["col"], win["row"], lam, win["steps"]) == ref
    _check_summary(_match(gpu_ctx, case, rng, L, lam), ref, win, case)
    gpu_ctx.release_grid(MAP)


@pytest.mark.gpu
def test_winner_in_the_extended_columns_pays_for_its_true_offset(gpu_ctx, oracle):
    """The peaks test's far-corner case: the winner sits in the extended columns (x > win_x) on the window's
    last row. A weak prior leaves it there, and its penalty is that of the true offsets."""
    L = 4
    _, _, st = oracle.search_step(0.05, np.array([5.7296]))
    wt = int(math.ceil(0.5 * RANGE[2] / st))
    case = synth.csm_case(6, init_error=(-13 * 0.05, -13 * 0.05, -wt * st))
    vol = P.volume(case, *RANGE, L)
    win = vol["win"]
    wx, wy, wt = win["win"]
    nt, nx, ny = win["shape"]
    w = _window(gpu_ctx, case, win, L)
    for lam in (sym(0.05, 0.05, 1.0), sym(0.05, 0.05, 1.0, 0.02, 0.1, -0.1)):
        ref, _ = P.prior(vol, case, lam)
        b = ref["best"]
        assert vol["cf"]["touchesBand"] == 0 and b["best_x"] > wx and b["best_y"] == ny - 1 - wy
        assert ref["penalty"] == P.penalty(ref["Q"], b["best_x"], b["best_y"], b["best_theta"]) > 0
        assert ref["penalty"] != P.penalty(ref["Q"], wx, b["best_y"], b["best_theta"])     # not the clipped column's
        assert gpu_ctx.score_window_prior(MAP, w, win["col"], win["row"], lam, win["steps"]) == ref
        _check_summary(_match(gpu_ctx, case, RANGE, L, lam), ref, win, case)
    # a strong prior pulls the winner out of the extended columns
    ref, _ = P.prior(vol, case, LAMBDAS["full"])
    assert ref["best"] != ref["unweighted"] and ref["unweighted"]["best_x"] > wx
    assert gpu_ctx.score_window_prior(MAP, w, win["col"], win["row"], LAMBDAS["full"], win["steps"]) == ref
    gpu_ctx.release_grid(MAP)


# (30, 4): the threshold takes the node of the peak at x = 0 out; a prior on x makes candidates of that
# node the best of the window by pk. (32, 3): nx / L != ny / L in the eligibility lookup.
@pytest.mark.gpu
@pytest.mark.parametrize("seed,L,lam,bites", [(30, 4, sym(4.0, 0.0, 0.0), True), (30, 4, sym(2.0, 0.0, 0.0, 0.0, 8.0), True),
                                              (32, 3, LAMBDAS["diag"], False), (32, 3, sym(8.0, 0.0, 0.0), False)])
def test_a_higher_pk_under_an_ineligible_node_is_not_chosen(gpu_ctx, oracle, seed, L, lam, bites):
    case = _elig_case(seed)
    thr, _ = _threshold_that_bites(oracle, case, L)
    vol, vol0 = P.volume(case, *ELIG_RANGE, L, 0.0, thr), P.volume(case, *ELIG_RANGE, L)
    win = vol["win"]
    wx, wy, wt = win["win"]
    nt, nx, ny = win["shape"]
    n = len(case["angles"])
    assert nx // L != ny // L and vol["cf"]["touchesBand"] == 0
    ref, _ = P.prior(vol, case, lam)
    ref0, _ = P.prior(vol0, case, lam)
    if bites:
        key = 32268 * vol["K"].astype(np.int64) + 499 * vol["S"].astype(np.int64)
        t, x, y = (a.astype(np.int64) for a in np.indices(vol["S"].shape))
        pk = key - P.penalty(ref["Q"], x - wx, y - wy, t - wt)
        ineligible = ~np.repeat(np.repeat(vol["CK"] / float(n) > thr, L, 1), L, 2)
        assert (pk[ineligible] > ref["penalised_key"]).any() and ref["best"] != ref0["best"]
    w = _window(gpu_ctx, case, win, L, known_thr=thr)
    assert gpu_ctx.score_window_prior(MAP, w, win["col"], win["row"], lam, win["steps"]) == ref
    _check_summary(_match(gpu_ctx, case, ELIG_RANGE, L, lam, known_rate_threshold=thr), ref, win, case)
    # the threshold-0 call on the same window still gives the threshold-0 winner
    w0 = gpu_ctx.make_window(w.n_theta, w.n_points, w.win_x, w.win_y, L, 1, api.host_min_known(w.n_points, 0.0), 0.0)
    assert gpu_ctx.score_window_prior(MAP, w0, win["col"], win["row"], lam, win["steps"]) == ref0
    gpu_ctx.release_grid(MAP)


@pytest.mark.gpu
def test_score_threshold_tests_the_raw_score_of_each_winner(gpu_ctx):
    """A threshold between the two winners' raw scores: the unweighted winner passes, the prior's does not,
    although its penalised score was the greater."""
    case, vol0 = _volume(0, 4)
    ref0 = _six(0, 4, "full")[2]
    assert ref0["best"]["score"] < ref0["unweighted"]["score"]
    thr = 0.5 * (ref0["best"]["score"] + ref0["unweighted"]["score"])
    vol = dict(vol0, score_thr=thr)
    ref, _ = P.prior(vol, case, LAMBDAS["full"])
    assert ref["best"] == P.ZERO and ref["penalty"] == 0 and ref["penalised_key"] == 0
    assert ref["unweighted"] == ref0["unweighted"] and ref["Q"] == ref0["Q"]
    win = vol["win"]
    w = _window(gpu_ctx, case, win, 4, score_thr=thr)
    assert gpu_ctx.score_window_prior(MAP, w, win["col"], win["row"], LAMBDAS["full"], win["steps"]) == ref
    out = _match(gpu_ctx, case, RANGE, 4, LAMBDAS["full"], score_threshold=thr)
    _check_summary(out, ref, win, case)
    assert out["summary"]["pose_found"] == 0 and out["summary"]["estimated_pose"] == [0.0] * 3
    gpu_ctx.release_grid(MAP)


@pytest.mark.gpu
def test_edge_band_windows_follow_the_closed_form_and_carry_the_flag(gpu_ctx):
    flagged = 0
    for (seed, L), name in zip(((50, 4), (52, 5), (53, 8), (55, 4)), ("full", "full", "diag", "indef")):
        case = synth.csm_case(seed, rows=256, cols=288, origin="low_edge", half_x=5.2, half_y=4.4,
                              init_error=(0.23, 0.19, 0.03))
        vol = P.volume(case, *RANGE, L)
        win = vol["win"]
        assert vol["cf"]["touchesBand"] == 1
        ref, _ = P.prior(vol, case, LAMBDAS[name])
        w = _window(gpu_ctx, case, win, L)
        band = gpu_ctx.score_window(MAP, w, win["col"], win["row"])["flags"] & Lb.FLAG_EDGE_BAND
        flagged += bool(band)
        got = gpu_ctx.score_window_prior(MAP, w, win["col"], win["row"], LAMBDAS[name], win["steps"])
        assert got == _with_band(ref, band)
        assert got["best"]["flags"] & Lb.FLAG_EDGE_BAND == got["unweighted"]["flags"] & Lb.FLAG_EDGE_BAND == band
        _check_summary(_match(gpu_ctx, case, RANGE, L, LAMBDAS[name]), ref, win, case, band)
        gpu_ctx.release_grid(MAP)
    assert flagged > 0          # the inputs must reach the edge-band path


@pytest.mark.gpu
def test_batch_in_chunks_equals_single_calls_and_leaks_no_state():
    base = api.debug_live_bytes()
    ctx = api.Context(0)
    maps, queries, cases, lams = {}, [], [], []
    names = list(LAMBDAS)
    for i in range(7):
        seed = 20 + i % 3
        n_beams, max_range = ((360, 5.7296), (1080, 8.0))[i % 2]
        rs = np.random.RandomState(100 + i)
        case = synth.csm_case(seed, n_beams=n_beams, max_range=max_range, rel_pose=(0.03 * (i % 4), 0.0, 0.02),
                              init_error=(0.3 * (rs.rand() - 0.5), 0.3 * (rs.rand() - 0.5), 0.05 * (rs.rand() - 0.5)))
        if seed not in maps:
            maps[seed] = MAP + 1 + len(maps)
            ctx.upload_grid(maps[seed], case["grid"])
        cases.append(case)
        queries.append(dict(map_id=maps[seed], geom=case["geom"], angles=case["angles"], ranges=case["ranges"],
                            rel_pose=case["rel_pose"], init_pose=case["init_pose"]))
        lams.append(LAMBDAS[names[i % 4]] * (6.0 + 1.5 * i))        # a prior of its own per query, strong enough to move winners 0.05 - 0.15 m off
    rng, L = (1.0, 1.0, math.radians(10)), 4
    before = ctx.correlative_match_batch(queries, *rng, L, 0.0, 0.0)
    vols = [P.volume(c, *rng, L) for c in cases]
    refs = [P.prior(v, c, lam)[0] for v, c, lam in zip(vols, cases, lams)]
    assert len({v["win"]["shape"] for v in vols}) > 1          # mixed windows
    assert sum(r["best"] != r["unweighted"] for r in refs) >= 2
    limit = 2 * max(_vol_bytes(v["win"]["shape"], L) for v in vols) + 1       # at most 2 windows per chunk
    ctx.enable_kernel_timing(True)
    ctx.reset_kernel_timing()
    got = ctx.correlative_match_prior_batch(queries, *rng, L, lams, scratch_limit_bytes=limit)
    chunks = ctx.kernel_time("prior_select")[1]
    ctx.enable_kernel_timing(False)
    assert chunks >= 4
    for q, c, v, ref, lam, g, b in zip(queries, cases, vols, refs, lams, got, before):
        band = b["raw"]["flags"] & Lb.FLAG_EDGE_BAND
        _check_summary(g, ref, v["win"], c, band)
        one = _match(ctx, c, rng, L, lam, map_id=q["map_id"])
        assert dict(one, summary=strip(one["summary"])) == dict(g, summary=strip(g["summary"]))
    assert [strip(o) for o in ctx.correlative_match_batch(queries, *rng, L, 0.0, 0.0)] == [strip(o) for o in before]

    # an error in query i: nothing is left pending, nothing is added, and the next call is right
    live = api.debug_live_bytes()
    bad = list(lams)
    bad[4] = lams[4] + np.array([[0.0, 1e-9, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])       # asymmetric
    with pytest.raises(api.CsmError) as e:
        ctx.correlative_match_prior_batch(queries, *rng, L, bad, scratch_limit_bytes=limit)
    assert e.value.code == Lb.CSM_EINVAL and api.debug_live_bytes() == live
    gone = [dict(q, map_id=MAP + 99) if i == 5 else q for i, q in enumerate(queries)]
    with pytest.raises(api.CsmError) as e:
        ctx.correlative_match_prior_batch(gone, *rng, L, lams, scratch_limit_bytes=limit)
    assert e.value.code == Lb.CSM_ENOENT and api.debug_live_bytes() == live
    again = ctx.correlative_match_prior_batch(queries, *rng, L, lams, scratch_limit_bytes=limit)
    assert [g["prior"] for g in again] == [g["prior"] for g in got] and api.debug_live_bytes() == live
    for m in maps.values():
        ctx.release_grid(m)
    ctx.close()
    assert api.debug_live_bytes() == base


@pytest.mark.gpu
def test_refusals_allocate_nothing(gpu_ctx):
    case, vol = _volume(0, 4)
    win, L = vol["win"], 4
    ref = _six(0, 4, "full")[2]
    w = _window(gpu_ctx, case, win, L)
    col, row, steps, lam = win["col"], win["row"], win["steps"], LAMBDAS["full"]
    assert gpu_ctx.score_window_prior(MAP, w, col, row, lam, steps) == ref      # workspaces at their size
    _check_summary(_match(gpu_ctx, case, RANGE, L, lam), ref, win, case)
    live = api.debug_live_bytes()

    def code(fn):
        with pytest.raises(api.CsmError) as e:
            fn()
        assert api.debug_live_bytes() == live
        return e.value.code

    nan, asym, huge = lam.copy(), lam.copy(), sym(1e30, 1.0, 1.0)
    nan[2, 2] = float("nan")
    asym[1, 0] += 1e-12
    wide = sym(1e6, 1.0, 1.0)           # fits int64, but 6 max|Q| d_max^2 >= 2^62 on this window
    assert P.quantise(wide, steps, w.n_points, P.d_max_of(win)) is None
    assert P.quantise(wide, steps, w.n_points, 1) is not None
    for bad in (nan, asym, huge, wide):
        assert code(lambda: gpu_ctx.score_window_prior(MAP, w, col, row, bad, steps)) == Lb.CSM_EINVAL
        assert code(lambda: _match(gpu_ctx, case, RANGE, L, bad)) == Lb.CSM_EINVAL
    assert code(lambda: gpu_ctx.score_window_prior(MAP, w, col, row, lam, steps, -1)) == Lb.CSM_EINVAL
    assert code(lambda: _match(gpu_ctx, case, RANGE, L, lam, scratch_limit_bytes=-1)) == Lb.CSM_EINVAL
    # the peaks' own refusals
    assert code(lambda: gpu_ctx.score_window_prior(MAP + 99, w, col, row, lam, steps)) == Lb.CSM_ENOENT
    assert code(lambda: _match(gpu_ctx, case, RANGE, L, lam, map_id=MAP + 99)) == Lb.CSM_ENOENT
    assert code(lambda: gpu_ctx.score_window_prior(MAP, w, col, row, lam, steps, 1024)) == Lb.CSM_EINVAL
    assert code(lambda: _match(gpu_ctx, case, RANGE, L, lam, scratch_limit_bytes=1024)) == Lb.CSM_EINVAL
    # a success after the failures, on workspaces that have their size: nothing is added
    assert gpu_ctx.score_window_prior(MAP, w, col, row, lam, steps) == ref
    assert api.debug_live_bytes() == live
    gpu_ctx.release_grid(MAP)
