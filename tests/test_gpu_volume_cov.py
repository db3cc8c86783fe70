"""GPU parity: pose covariance from the whole score volume (csm_score_window_moments,
csm_correlative_covariance, csm_correlative_covariance_batch) against tests/volume_reference.py. Bar: every
integer equal, every double bit-equal; nothing carries a tolerance."""
import functools
import math

import numpy as np
import pytest

import peaks_reference as PR
import volume_reference as VR
from csm_hip import _lib as Lb, api, synth
from test_gpu_peaks import CASES, ELIG_RANGE, RANGE, _elig_case, _threshold_that_bites, _uniform_case, _vol_bytes

pytestmark = pytest.mark.gpu

TAUS = (0.005, 0.02)
MAP = 800


@functools.lru_cache(maxsize=None)
def _case(seed):
    return synth.csm_case(seed)


def _reference(case, rng, L, tau, score_thr=0.0, known_thr=0.0):
    return VR.summary(case, *rng, L, tau, score_thr, known_thr)


@functools.lru_cache(maxsize=None)
def _six(seed, L, tau):
    """(case, reference, window) of one of the six cases: computed once, shared, never changed."""
    case = _case(seed)
    if seed in (1, 4):          # the Jacobian of MoveBackward needs a sensor off the robot's origin
        case = dict(case, rel_pose=(0.21, -0.13, 0.3))
    return (case,) + _reference(case, RANGE, L, tau)


def _window(ctx, case, win, L, score_thr=0.0, known_thr=0.0, map_id=MAP):
    """Uploads the map and returns the csm_window of the reference's window."""
    wx, wy, wt = win["win"]
    ctx.upload_grid(map_id, case["grid"])
    ctx.build_pyramid(map_id, [1, L])
    n = len(case["angles"])
    return ctx.make_window(2 * wt + 1, n, wx, wy, L, 1 if L > 1 else 0, api.host_min_known(n, known_thr), score_thr)


def _covariance(ctx, case, rng, L, tau, map_id=MAP, **kw):
    return ctx.correlative_covariance(map_id, case["geom"], case["angles"], case["ranges"], case["rel_pose"],
                                      case["init_pose"], *rng, L, tau, **kw)


def _with_band(ref_moments, band):
    return dict(ref_moments, best=dict(ref_moments["best"], flags=ref_moments["best"]["flags"] | band))


def _check_summary(out, ref, win, case, band=0):
    """A csm_volume_summary against the reference: moments, the three double arrays, the poses."""
    assert out["moments"] == _with_band(ref["moments"], band)
    assert out["mean_offset"] == ref["mean_offset"]                     # bit-exact doubles
    assert out["sensor_covariance"] == ref["sensor_covariance"]
    assert out["covariance"] == ref["covariance"]
    s = out["summary"]
    assert s["raw"] == out["moments"]["best"] and s["pose_found"] == out["moments"]["best"]["found"]
    assert (s["win_x"], s["win_y"], s["win_theta"]) == win["win"]
    assert s["candidates"] == int(np.prod(win["shape"]))
    if ref["estimated_pose"] is not None:
        best, est = PR.poses_of(ref["moments"]["best"], win, case["rel_pose"])
        assert s["best_sensor_pose"] == best and s["estimated_pose"] == est == ref["estimated_pose"]


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("seed,L", CASES)
def test_six_cases_moments_covariance_and_winner(gpu_ctx, seed, L, tau):
    case, ref, win = _six(seed, L, tau)
    m = ref["moments"]
    assert m["best"]["found"] == 1 and m["support"] >= 1 and m["m0"] >= 1 << 24
    w = _window(gpu_ctx, case, win, L)
    before = gpu_ctx.correlative_match(MAP, case["geom"], case["angles"], case["ranges"], case["rel_pose"],
                                       case["init_pose"], *RANGE, L)
    got = gpu_ctx.score_window_moments(MAP, w, win["col"], win["row"], tau)
    assert got == m
    assert got["best"] == gpu_ctx.score_window_peaks(MAP, w, win["col"], win["row"], 1)[0]
    out = _covariance(gpu_ctx, case, RANGE, L, tau)
    _check_summary(out, ref, win, case)
    if any(case["rel_pose"][:2]):
        assert out["covariance"] != out["sensor_covariance"]
    after = gpu_ctx.correlative_match(MAP, case["geom"], case["angles"], case["ranges"], case["rel_pose"],
                                      case["init_pose"], *RANGE, L)
    strip = lambda o: {k: v for k, v in o.items() if not k.endswith("_us")}
    assert strip(before) == strip(after) and after["raw"] == got["best"]
    gpu_ctx.release_grid(MAP)


def test_both_regimes_are_covered():
    """The six cases at the two temperatures reach a support of tens and of thousands of candidates, with
    and without weight on the window's faces."""
    refs = {(seed, tau): _six(seed, L, tau)[1]["moments"] for seed, L in CASES for tau in TAUS}
    assert min(m["support"] for m in refs.values()) < 64 < 1000 < max(m["support"] for m in refs.values())
    assert any(m["border_support"] == 0 for m in refs.values())
    assert any(m["border_support"] > 0 for m in refs.values())
    assert any(m["m1"] != [0, 0, 0] for m in refs.values())


def test_winner_at_the_far_corner_of_the_extended_domain(gpu_ctx, oracle):
    """The peaks test's far-corner case: the winner sits in the extended columns (x > win_x), on the window's
    last row and one slice short of the last. No candidate lies past it in y, two columns and one slice
    do in x and theta: the y moment is <= 0 at any temperature, and once the support is wide (tau = 0.02)
    the x moment is negative too."""
    L = 4
    _, _, st = oracle.search_step(0.05, np.array([5.7296]))
    wt = int(math.ceil(0.5 * RANGE[2] / st))
    case = synth.csm_case(6, init_error=(-13 * 0.05, -13 * 0.05, -wt * st))
    refs = [_reference(case, RANGE, L, tau) for tau in TAUS]
    win = refs[0][1]
    w = _window(gpu_ctx, case, win, L)
    for tau, (ref, _) in zip(TAUS, refs):
        m = ref["moments"]
        wx, wy, wt = win["win"]
        nt, nx, ny = win["shape"]
        b = m["best"]
        assert b["best_x"] > wx and b["best_y"] == ny - 1 - wy and b["best_theta"] + 2 > wt
        assert m["m1"][1] <= 0 and m["border_support"] >= 1
        assert gpu_ctx.score_window_moments(MAP, w, win["col"], win["row"], tau) == m
        _check_summary(_covariance(gpu_ctx, case, RANGE, L, tau), ref, win, case)
    wide = refs[-1][0]["moments"]
    assert wide["m1"][0] < 0 and wide["m1"][1] < 0 and wide["m2"][2] < 0       # signed sums
    gpu_ctx.release_grid(MAP)


@pytest.mark.parametrize("L", [1, 2])
def test_uniform_map_thousands_at_full_weight_over_several_workgroups(gpu_ctx, L):
    case = _uniform_case()
    rng = (1.2, 1.2, math.radians(24))
    tau = 0.02
    ref, win = _reference(case, rng, L, tau)
    m = ref["moments"]
    assert int(np.prod(win["shape"])) > 8192                      # more than one workgroup per window
    assert m["best"]["tie_count"] > 1000 and m["m0"] >= m["best"]["tie_count"] << 24
    w = _window(gpu_ctx, case, win, L)
    assert gpu_ctx.score_window_moments(MAP, w, win["col"], win["row"], tau) == m
    _check_summary(_covariance(gpu_ctx, case, rng, L, tau), ref, win, case)
    gpu_ctx.release_grid(MAP)


@pytest.mark.parametrize("seed,L", [(32, 3), (30, 4)])
def test_ineligible_candidates_weigh_nothing(gpu_ctx, oracle, seed, L):
    case = _elig_case(seed)
    thr, _ = _threshold_that_bites(oracle, case, L)
    tau = 0.02
    ref, win = _reference(case, ELIG_RANGE, L, tau, 0.0, thr)
    ref0, _ = _reference(case, ELIG_RANGE, L, tau)
    assert ref["moments"] != ref0["moments"] and ref["moments"]["support"] < ref0["moments"]["support"]
    w = _window(gpu_ctx, case, win, L, known_thr=thr)
    assert gpu_ctx.score_window_moments(MAP, w, win["col"], win["row"], tau) == ref["moments"]
    _check_summary(_covariance(gpu_ctx, case, ELIG_RANGE, L, tau, known_rate_threshold=thr), ref, win, case)
    # the threshold-0 call on the same window still gives the threshold-0 moments
    w0 = gpu_ctx.make_window(w.n_theta, w.n_points, w.win_x, w.win_y, L, 1, api.host_min_known(w.n_points, 0.0), 0.0)
    assert gpu_ctx.score_window_moments(MAP, w0, win["col"], win["row"], tau) == ref0["moments"]
    gpu_ctx.release_grid(MAP)


def test_score_threshold_above_the_winner_finds_nothing(gpu_ctx):
    case, L, tau = _case(0), 4, 0.02
    ref0, win = _reference(case, RANGE, L, tau)
    thr = ref0["moments"]["best"]["score"]          # the test is score > threshold
    ref, _ = _reference(case, RANGE, L, tau, thr)
    m = ref["moments"]
    assert m["best"]["found"] == 0 and m["m0"] == 0 and m["support"] == 0
    w = _window(gpu_ctx, case, win, L, score_thr=thr)
    got = gpu_ctx.score_window_moments(MAP, w, win["col"], win["row"], tau)
    assert got == m
    assert got["m1"] == [0] * 3 and got["m2"] == [0] * 6 and got["border_support"] == 0
    out = _covariance(gpu_ctx, case, RANGE, L, tau, score_threshold=thr)
    _check_summary(out, ref, win, case)
    assert out["summary"]["pose_found"] == 0 and out["covariance"] == [0.0] * 9
    gpu_ctx.release_grid(MAP)


def test_edge_band_windows_follow_the_closed_form_and_carry_the_flag(gpu_ctx):
    flagged = 0
    for seed, L in ((50, 4), (52, 5), (53, 8), (55, 4)):
        case = synth.csm_case(seed, rows=256, cols=288, origin="low_edge", half_x=5.2, half_y=4.4,
                              init_error=(0.23, 0.19, 0.03))
        tau = TAUS[seed % 2]
        ref, win = _reference(case, RANGE, L, tau)
        w = _window(gpu_ctx, case, win, L)
        band = gpu_ctx.score_window(MAP, w, win["col"], win["row"])["flags"] & Lb.FLAG_EDGE_BAND
        flagged += bool(band)
        assert gpu_ctx.score_window_moments(MAP, w, win["col"], win["row"], tau) == _with_band(ref["moments"], band)
        _check_summary(_covariance(gpu_ctx, case, RANGE, L, tau), ref, win, case, band)
        gpu_ctx.release_grid(MAP)
    assert flagged > 0          # the inputs must reach the edge-band path


def test_batch_in_chunks_equals_single_calls_and_leaks_no_state():
    base = api.debug_live_bytes()
    ctx = api.Context(0)
    maps, queries, cases = {}, [], []
    for i in range(12):
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
    assert len(maps) == 3
    strip = lambda o: {k: v for k, v in o.items() if not k.endswith("_us")}
    for rng, L, tau in (((1.0, 1.0, math.radians(10)), 4, 0.02), ((0.8, 1.2, math.radians(6)), 3, 0.005)):
        before = ctx.correlative_match_batch(queries, *rng, L, 0.0, 0.0)
        refs = [_reference(c, rng, L, tau) for c in cases]
        assert len({r[1]["shape"] for r in refs}) > 1          # mixed windows
        limit = 4 * max(_vol_bytes(r[1]["shape"], L) for r in refs) + 1       # at most 4 windows per chunk
        ctx.enable_kernel_timing(True)
        ctx.reset_kernel_timing()
        got = ctx.correlative_covariance_batch(queries, *rng, L, tau, scratch_limit_bytes=limit)
        chunks = ctx.kernel_time("volume_moments")[1]
        ctx.enable_kernel_timing(False)
        assert chunks >= 3
        for q, c, (ref, win), g, b in zip(queries, cases, refs, got, before):
            band = b["raw"]["flags"] & Lb.FLAG_EDGE_BAND
            _check_summary(g, ref, win, c, band)
            one = _covariance(ctx, c, rng, L, tau, map_id=q["map_id"])
            assert dict(one, summary=strip(one["summary"])) == dict(g, summary=strip(g["summary"]))
        after = ctx.correlative_match_batch(queries, *rng, L, 0.0, 0.0)
        assert [strip(o) for o in before] == [strip(o) for o in after]
    for m in maps.values():
        ctx.release_grid(m)
    ctx.close()
    assert api.debug_live_bytes() == base


def test_errors_and_live_bytes(gpu_ctx):
    case, L, tau = _case(0), 4, 0.02
    ref, win = _reference(case, RANGE, L, tau)
    w = _window(gpu_ctx, case, win, L)
    col, row = win["col"], win["row"]
    assert gpu_ctx.score_window_moments(MAP, w, col, row, tau) == ref["moments"]      # workspaces at their size
    _check_summary(_covariance(gpu_ctx, case, RANGE, L, tau), ref, win, case)
    live = api.debug_live_bytes()

    def code(fn):
        with pytest.raises(api.CsmError) as e:
            fn()
        assert api.debug_live_bytes() == live
        return e.value.code

    for bad in (0.0, -0.02, float("nan")):
        assert code(lambda: gpu_ctx.score_window_moments(MAP, w, col, row, bad)) == Lb.CSM_EINVAL
        assert code(lambda: _covariance(gpu_ctx, case, RANGE, L, bad)) == Lb.CSM_EINVAL
    # 1441 x 801 x 801 candidates of 8 beams: refused by the range check before any work (no hit index is read)
    big = gpu_ctx.make_window(1441, 8, 400, 400, 1, 0, 1, 0.0)
    none = np.zeros(1, np.int32)
    assert 1441 * 801 * 801 * 1440 ** 2 << 24 >= 1 << 63
    assert code(lambda: gpu_ctx.score_window_moments(MAP, big, none, none, tau)) == Lb.CSM_EINVAL
    assert code(lambda: gpu_ctx.score_window_moments(MAP + 99, w, col, row, tau)) == Lb.CSM_ENOENT
    assert code(lambda: _covariance(gpu_ctx, case, RANGE, L, tau, map_id=MAP + 99)) == Lb.CSM_ENOENT
    assert code(lambda: gpu_ctx.score_window_moments(MAP, w, col, row, tau, 1024)) == Lb.CSM_EINVAL
    assert code(lambda: _covariance(gpu_ctx, case, RANGE, L, tau, scratch_limit_bytes=1024)) == Lb.CSM_EINVAL
    # a success after the failures, on workspaces that have their size: nothing is added
    assert gpu_ctx.score_window_moments(MAP, w, col, row, tau) == ref["moments"]
    assert api.debug_live_bytes() == live
    gpu_ctx.release_grid(MAP)
