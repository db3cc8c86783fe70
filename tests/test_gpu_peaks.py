"""GPU parity: the K best distinct poses per window (csm_score_window_peaks, csm_correlative_peaks,
csm_correlative_peaks_batch) against tests/peaks_reference.py. Bar: every record equal field by field,
the f64 score bit for bit; poses equal to those rebuilt from the indices."""
import math

import numpy as np
import pytest

import peaks_reference as PR
from csm_hip import _lib as Lb, api, synth

pytestmark = pytest.mark.gpu

CASES = [(0, 4), (1, 4), (2, 1), (3, 5), (4, 3), (5, 8)]
RANGE = (1.0, 1.0, math.radians(10))
K_MAX, EXCL = 4, (3, 3, 2)
MAP = 700


def _window_peaks(ctx, case, rng, L, k_max, excl, score_thr=0.0, map_id=MAP, known_thr=0.0):
    """score_window_peaks on the case's window with host-projected hit indices; uploads the map."""
    ref, cf, win = PR.peaks(case, *rng, L, k_max, excl, score_thr, known_thr)
    wx, wy, wt = win["win"]
    ctx.upload_grid(map_id, case["grid"])
    ctx.build_pyramid(map_id, [1, L])
    n = len(case["angles"])
    w = ctx.make_window(2 * wt + 1, n, wx, wy, L, 1 if L > 1 else 0, api.host_min_known(n, known_thr), score_thr)
    got = ctx.score_window_peaks(map_id, w, win["col"], win["row"], k_max, excl)
    return got, ref, cf, win, w


def _match_peaks(ctx, case, rng, L, k_max, excl, map_id=MAP, **kw):
    return ctx.correlative_peaks(map_id, case["geom"], case["angles"], case["ranges"], case["rel_pose"],
                                 case["init_pose"], *rng, L, k_max, excl, **kw)


@pytest.mark.parametrize("seed,L", CASES)
def test_six_cases_records_poses_and_winner(gpu_ctx, seed, L):
    case = synth.csm_case(seed)
    got, ref, cf, win, w = _window_peaks(gpu_ctx, case, RANGE, L, K_MAX, EXCL)
    assert cf["touchesBand"] == 0 and len(ref) == K_MAX
    assert got == ref                                       # field by field, score bits included
    single = gpu_ctx.score_window(MAP, w, win["col"], win["row"])
    assert not single["flags"] & (Lb.FLAG_EDGE_BAND | Lb.FLAG_LITERAL)
    assert got[0] == single
    out = _match_peaks(gpu_ctx, case, RANGE, L, K_MAX, EXCL)
    assert [o["raw"] for o in out] == ref
    for o, r in zip(out, ref):
        best, est = PR.poses_of(r, win, case["rel_pose"])
        assert o["pose_found"] == 1
        assert o["best_sensor_pose"] == best and o["estimated_pose"] == est       # bit-exact doubles
        assert (o["win_x"], o["win_y"], o["win_theta"]) == win["win"]
        assert o["candidates"] == int(np.prod(win["shape"]))
    m = gpu_ctx.correlative_match(MAP, case["geom"], case["angles"], case["ranges"], case["rel_pose"],
                                  case["init_pose"], *RANGE, L)
    assert out[0]["raw"] == m["raw"]
    assert out[0]["best_sensor_pose"] == m["best_sensor_pose"] and out[0]["estimated_pose"] == m["estimated_pose"]
    gpu_ctx.release_grid(MAP)


@pytest.mark.parametrize("seed,L", [(2, 1), (0, 4)])
def test_plain_top_k_whole_window_box_and_threshold(gpu_ctx, seed, L):
    case = synth.csm_case(seed)
    got, ref, cf, win, w = _window_peaks(gpu_ctx, case, RANGE, L, 16, (0, 0, 0))
    assert len(ref) == 16 and got == ref
    keys = [r["key"] for r in got]
    assert keys == sorted(keys, reverse=True)
    # an exclusion box over the whole window leaves nothing after the first peak
    nt, nx, ny = win["shape"]
    assert gpu_ctx.score_window_peaks(MAP, w, win["col"], win["row"], 16, (nx, ny, nt)) == ref[:1]
    # a threshold between the reference's peak 1 and peak 2 ends the list after two
    ref4, _, _ = PR.peaks(case, *RANGE, L, K_MAX, EXCL)
    assert ref4[1]["score"] > ref4[2]["score"]
    thr = 0.5 * (ref4[1]["score"] + ref4[2]["score"])
    assert ref4[1]["score"] > thr > ref4[2]["score"]
    out = _match_peaks(gpu_ctx, case, RANGE, L, K_MAX, EXCL, score_threshold=thr)
    assert [o["raw"] for o in out] == ref4[:2]
    gpu_ctx.release_grid(MAP)


def test_peak_at_the_far_corner_clips_the_exclusion_box(gpu_ctx, oracle):
    """The scan's true pose lies past +win in x and y and at the last slices: the first peak sits in the
    extended columns (x > win_x) on the window's last row, so its exclusion box is clipped at the border."""
    L = 4
    _, _, st = oracle.search_step(0.05, np.array([5.7296]))
    wt = int(math.ceil(0.5 * RANGE[2] / st))
    case = synth.csm_case(6, init_error=(-13 * 0.05, -13 * 0.05, -wt * st))
    got, ref, cf, win, w = _window_peaks(gpu_ctx, case, RANGE, L, K_MAX, EXCL)
    wx, wy, wt = win["win"]
    nt, nx, ny = win["shape"]
    assert cf["touchesBand"] == 0 and len(ref) == K_MAX
    assert ref[0]["best_x"] > wx and ref[0]["best_y"] == ny - 1 - wy and ref[0]["best_theta"] + EXCL[2] > wt
    assert got == ref
    assert [o["raw"] for o in _match_peaks(gpu_ctx, case, RANGE, L, K_MAX, EXCL)] == ref
    gpu_ctx.release_grid(MAP)


def _uniform_case():
    """96 x 96 cells, every known cell the same value: candidates with equal K tie in key AND in f64 score."""
    grid = np.zeros((96, 96), np.uint16)
    grid[8:88, 8:88] = 30000
    grid[30:40, 50:70] = 0
    n = 90
    ang = -math.pi + 2 * math.pi * np.arange(n) / n
    rng = np.full(n, 1.1)
    rng[::3] = 1.4
    rng[0] = 1.5
    return dict(grid=grid, geom=(0.05, -2.4 + 0.0137, -2.4 - 0.0219), angles=ang, ranges=rng,
                rel_pose=(0.0, 0.0, 0.0), init_pose=(0.31, -0.2, 0.1))


@pytest.mark.parametrize("L", [1, 2])
def test_ties_resolve_in_traversal_order(gpu_ctx, L):
    """More than 8192 candidates: the tie set of a round spreads over several workgroups' chunks."""
    case = _uniform_case()
    rng = (1.2, 1.2, math.radians(24))
    got, ref, cf, win, w = _window_peaks(gpu_ctx, case, rng, L, 6, (1, 1, 1))
    assert int(np.prod(win["shape"])) > 8192 and cf["touchesBand"] == 0
    assert len(ref) == 6 and all(r["tie_count"] > 1 for r in ref)
    assert all(r["flags"] & Lb.FLAG_KEY_TIE for r in ref)
    assert got == ref
    assert [o["raw"] for o in _match_peaks(gpu_ctx, case, rng, L, 6, (1, 1, 1))] == ref
    gpu_ctx.release_grid(MAP)


# ---- eligibility: a known-rate threshold that takes higher-key candidates out ----

ELIG_RANGE = (0.8, 1.4, math.radians(8))       # nx / L != ny / L for L = 3 (6 x 10 nodes) and L = 4 (5 x 8)


def _elig_case(seed):
    return synth.csm_case(seed, interior_unknown=0.25, rel_pose=(0.04, -0.02, 0.01))


def _threshold_that_bites(oracle, case, L):
    """The smallest known rate among the coarse nodes of the threshold-0 peaks: as the threshold it makes
    that node, and with it a peak of the threshold-0 list, ineligible (the test is known rate > threshold)."""
    ref0, _, win = PR.peaks(case, *ELIG_RANGE, L, K_MAX, EXCL)
    _, S, K, CK = oracle.csm_closed_form(case, *ELIG_RANGE, L, dump=True)
    wx, wy, wt = win["win"]
    n = len(case["angles"])
    thr = min(int(CK[r["best_theta"] + wt, (r["best_x"] + wx) // L, (r["best_y"] + wy) // L]) for r in ref0) / float(n)
    ref, _, _ = PR.peaks(case, *ELIG_RANGE, L, K_MAX, EXCL, 0.0, thr)
    # the preconditions: the lists differ, and an ineligible candidate outranks a returned peak
    assert len(ref) == K_MAX and ref != ref0
    key = 32268 * K.astype(np.int64) + 499 * S.astype(np.int64)
    ineligible = ~np.repeat(np.repeat(CK / float(n) > thr, L, 1), L, 2)
    assert (key[ineligible] > ref[-1]["key"]).any()
    assert 1 < api.host_min_known(n, thr) <= n
    return thr, ref0


@pytest.mark.parametrize("seed,L", [(32, 3), (30, 4)])
def test_known_rate_threshold_takes_higher_keys_out(gpu_ctx, oracle, seed, L):
    case = _elig_case(seed)
    thr, ref0 = _threshold_that_bites(oracle, case, L)
    got, ref, cf, win, w = _window_peaks(gpu_ctx, case, ELIG_RANGE, L, K_MAX, EXCL, known_thr=thr)
    nt, nx, ny = win["shape"]
    assert nx // L != ny // L and cf["touchesBand"] == 0
    assert got == ref and got != ref0
    out = _match_peaks(gpu_ctx, case, ELIG_RANGE, L, K_MAX, EXCL, known_rate_threshold=thr)
    assert [o["raw"] for o in out] == ref
    # the threshold-0 call on the same window still gives the threshold-0 list
    w0 = gpu_ctx.make_window(w.n_theta, w.n_points, w.win_x, w.win_y, L, 1, api.host_min_known(w.n_points, 0.0), 0.0)
    assert gpu_ctx.score_window_peaks(MAP, w0, win["col"], win["row"], K_MAX, EXCL) == ref0
    gpu_ctx.release_grid(MAP)


def test_known_rate_threshold_in_a_batch(gpu_ctx, oracle):
    L = 3
    cases = [_elig_case(seed) for seed in (32, 30, 33, 32)]
    thr, _ = _threshold_that_bites(oracle, cases[0], L)
    queries = []
    for i, c in enumerate(cases):
        gpu_ctx.upload_grid(MAP + 10 + i, c["grid"])
        queries.append(dict(map_id=MAP + 10 + i, geom=c["geom"], angles=c["angles"], ranges=c["ranges"],
                            rel_pose=c["rel_pose"], init_pose=c["init_pose"]))
    refs = [PR.peaks(c, *ELIG_RANGE, L, K_MAX, EXCL, 0.0, thr)[0] for c in cases]
    refs0 = [PR.peaks(c, *ELIG_RANGE, L, K_MAX, EXCL)[0] for c in cases]
    assert sum(a != b for a, b in zip(refs, refs0)) >= 2
    got = gpu_ctx.correlative_peaks_batch(queries, *ELIG_RANGE, L, K_MAX, EXCL, known_rate_threshold=thr)
    assert [[o["raw"] for o in g] for g in got] == refs
    for i in range(len(cases)):
        gpu_ctx.release_grid(MAP + 10 + i)


# ---- the negative edge band ----

def test_edge_band_windows_follow_the_closed_form_and_carry_the_flag(gpu_ctx):
    """The room's low walls sit 1-2 cells inside the map's low edges: coarse reads fall in the negative
    edge band. The peaks are the closed form's (tests/peaks_reference.py) whatever the single-best search
    did, and every record carries FLAG_EDGE_BAND exactly when the single-best record does."""
    flagged = 0
    for seed, L in ((50, 4), (52, 5), (53, 8), (55, 4)):
        case = synth.csm_case(seed, rows=256, cols=288, origin="low_edge", half_x=5.2, half_y=4.4,
                              init_error=(0.23, 0.19, 0.03))
        got, ref, cf, win, w = _window_peaks(gpu_ctx, case, RANGE, L, K_MAX, EXCL)
        assert cf["touchesBand"] == 1 and len(ref) == K_MAX
        single = gpu_ctx.score_window(MAP, w, win["col"], win["row"])
        band = single["flags"] & Lb.FLAG_EDGE_BAND
        flagged += bool(band)
        assert got == [dict(r, flags=r["flags"] | band) for r in ref]
        out = _match_peaks(gpu_ctx, case, RANGE, L, K_MAX, EXCL)
        assert [o["raw"] for o in out] == got
        gpu_ctx.release_grid(MAP)
    assert flagged > 0          # the inputs must reach the edge-band path


def _vol_bytes(shape, L):
    a = lambda v: (v + 255) & ~255
    total = int(np.prod(shape))
    return a(4 * total) + a(2 * total) + (a(2 * total // (L * L)) if L > 1 else 0)


def test_batch_in_chunks_equals_single_calls_and_leaks_no_state(gpu_ctx):
    maps = {}
    queries, cases = [], []
    for i in range(12):
        seed = 20 + i % 3
        n_beams, max_range = ((360, 5.7296), (1080, 8.0))[i % 2]
        rs = np.random.RandomState(100 + i)
        case = synth.csm_case(seed, n_beams=n_beams, max_range=max_range, rel_pose=(0.03 * (i % 4), 0.0, 0.02),
                              init_error=(0.3 * (rs.rand() - 0.5), 0.3 * (rs.rand() - 0.5), 0.05 * (rs.rand() - 0.5)))
        if seed not in maps:
            maps[seed] = MAP + 1 + len(maps)
            gpu_ctx.upload_grid(maps[seed], case["grid"])
        cases.append(case)
        queries.append(dict(map_id=maps[seed], geom=case["geom"], angles=case["angles"], ranges=case["ranges"],
                            rel_pose=case["rel_pose"], init_pose=case["init_pose"]))
    assert len(maps) == 3
    for rng, L in (((1.0, 1.0, math.radians(10)), 4), ((0.8, 1.2, math.radians(6)), 3)):
        before = gpu_ctx.correlative_match_batch(queries, *rng, L, 0.0, 0.0)
        refs = [PR.peaks(c, *rng, L, K_MAX, EXCL) for c in cases]
        assert len({r[2]["shape"] for r in refs}) > 1          # mixed windows
        limit = 4 * max(_vol_bytes(r[2]["shape"], L) for r in refs) + 1       # at most 4 windows per chunk
        gpu_ctx.enable_kernel_timing(True)
        gpu_ctx.reset_kernel_timing()
        got = gpu_ctx.correlative_peaks_batch(queries, *rng, L, K_MAX, EXCL, scratch_limit_bytes=limit)
        chunks = gpu_ctx.kernel_time("peaks_select")[1]
        gpu_ctx.enable_kernel_timing(False)
        assert chunks >= 3
        for q, c, (ref, cf, win), g in zip(queries, cases, refs, got):
            assert [o["raw"] for o in g] == ref
            one = gpu_ctx.correlative_peaks(q["map_id"], c["geom"], c["angles"], c["ranges"], c["rel_pose"],
                                            c["init_pose"], *rng, L, K_MAX, EXCL)
            for a, b in zip(g, one):
                a, b = dict(a), dict(b)
                for t in ("input_setup_us", "optimization_us"):
                    a.pop(t), b.pop(t)
                assert a == b
            assert len(g) == len(one)
        after = gpu_ctx.correlative_match_batch(queries, *rng, L, 0.0, 0.0)
        strip = lambda out: [{k: v for k, v in o.items() if not k.endswith("_us")} for o in out]
        assert strip(before) == strip(after)
        for g, b in zip(got, before):
            # peak records never carry FLAG_PROJ_DELTA (the batch's note that it redid a projection)
            if not b["raw"]["flags"] & (Lb.FLAG_EDGE_BAND | Lb.FLAG_LITERAL):
                assert g[0]["raw"] == dict(b["raw"], flags=b["raw"]["flags"] & ~Lb.FLAG_PROJ_DELTA)
    for m in maps.values():
        gpu_ctx.release_grid(m)


def test_errors_and_live_bytes(gpu_ctx):
    case = synth.csm_case(0)
    got, ref, cf, win, w = _window_peaks(gpu_ctx, case, RANGE, 4, K_MAX, EXCL)      # workspaces at their size
    assert got == ref
    live = api.debug_live_bytes()

    def code(fn):
        with pytest.raises(api.CsmError) as e:
            fn()
        assert api.debug_live_bytes() == live
        return e.value.code

    col, row = win["col"], win["row"]
    assert code(lambda: gpu_ctx.score_window_peaks(MAP, w, col, row, 0)) == Lb.CSM_EINVAL
    assert code(lambda: gpu_ctx.score_window_peaks(MAP, w, col, row, 17)) == Lb.CSM_EINVAL
    assert code(lambda: gpu_ctx.score_window_peaks(MAP, w, col, row, 4, (0, -1, 0))) == Lb.CSM_EINVAL
    assert code(lambda: _match_peaks(gpu_ctx, case, RANGE, 4, 4, (-1, 0, 0))) == Lb.CSM_EINVAL
    assert code(lambda: gpu_ctx.score_window_peaks(MAP + 99, w, col, row, 4)) == Lb.CSM_ENOENT
    assert code(lambda: _match_peaks(gpu_ctx, case, RANGE, 4, 4, EXCL, map_id=MAP + 99)) == Lb.CSM_ENOENT
    assert code(lambda: gpu_ctx.score_window_peaks(MAP, w, col, row, 4, EXCL, 1024)) == Lb.CSM_EINVAL
    assert code(lambda: _match_peaks(gpu_ctx, case, RANGE, 4, 4, EXCL, scratch_limit_bytes=1024)) == Lb.CSM_EINVAL
    # a success after the failures, on workspaces that have their size: nothing is added
    assert gpu_ctx.score_window_peaks(MAP, w, col, row, K_MAX, EXCL) == ref
    assert api.debug_live_bytes() == live
    gpu_ctx.release_grid(MAP)
    # a context of its own: everything a successful call allocated goes with it
    base = api.debug_live_bytes()
    ctx = api.Context(0)
    got2, ref2, _, _, _ = _window_peaks(ctx, case, RANGE, 4, K_MAX, EXCL)
    assert got2 == ref2
    assert api.debug_live_bytes() != base
    ctx.release_grid(MAP)
    ctx.close()
    assert api.debug_live_bytes() == base
