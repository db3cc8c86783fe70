"""GPU parity of the box-maximum levels (k_boxmax_batch) the searches prune with: every level a
context holds, downloaded and compared byte for byte with the plain reference of
tests/boxmax_cases.py (held by test_cpu_boxmax_cases.py), at the tile edges, with pad columns, for
several maps in one launch, after the base map changed, at the limits of the window size -- and
after a batched call that failed: such a call must leave no level that reads as built and was
never written."""
import math

import numpy as np
import pytest

import boxmax_cases as BC
from csm_hip import _lib as L, api, synth

pytestmark = pytest.mark.gpu

BNB_RANGES = (1.0, 1.0, 0.25)
BNB_THRESHOLDS = (0.3, 0.5)
CSM_RANGES = (1.0, 1.0, math.radians(10))


def _refused(code, call, *args):
    with pytest.raises(api.CsmError) as err:
        call(*args)
    assert err.value.code == code, err.value


def _check_levels(ctx, map_id, grid, wins, must_exist=True):
    """Level i of the map is box-max(wins[i]) of grid -- or, where a level may be missing, is refused
    with CSM_ENOENT. Never anything else. Returns the indices that downloaded."""
    present = []
    for i, win in enumerate(wins):
        try:
            got = ctx.download_level(map_id, i)
        except api.CsmError as e:
            assert e.code == L.CSM_ENOENT and not must_exist, (i, win, e)
            continue
        want = grid if win == 1 else BC.boxmax_plain(grid, win)
        bad = np.argwhere(got != want)
        assert bad.size == 0, "level %d (window %d): %d cells differ, first at %s: got %d, want %d; got is %s" % (
            i, win, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])],
            "all zero" if not got.any() else "not all zero")
        present.append(i)
    return present


# ---------------------------------------------------------------- a. every case, single build


@pytest.mark.parametrize("rows,cols,win,fill", BC.CASES, ids=BC.CASE_IDS)
def test_level_matches_plain_reference(gpu_ctx, rows, cols, win, fill):
    """Includes the limits that are accepted: W = rows, W = cols, W = 64."""
    grid, want = BC.case_arrays(rows, cols, win, fill)
    gpu_ctx.upload_grid(7100, grid)
    try:
        gpu_ctx.build_pyramid(7100, [1, win])
        got = gpu_ctx.download_level(7100, 1)
        assert np.array_equal(gpu_ctx.download_level(7100, 0), grid)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
    finally:
        gpu_ctx.release_grid(7100)


# ---------------------------------------------------------------- b. several levels and maps in one launch


def test_many_maps_and_levels_in_one_launch(gpu_ctx):
    """One launch grid sized by the largest map (200 rows, pitch 200): three of the four maps end
    before it on at least one axis (the kernel's early return), 33 columns leave 7 pad columns."""
    shapes = [(20, 24), (33, 200), (200, 33), (97, 129)]
    wins = [1, 2, 3, 8, 16]
    ids = [7110 + k for k in range(len(shapes))]
    grids = [BC.make_grid(r, c, 16, "random") for r, c in shapes]
    boxmax_before = gpu_ctx.kernel_time("boxmax")[1]
    gpu_ctx.enable_kernel_timing(True)
    try:
        for i, g in zip(ids, grids):
            gpu_ctx.upload_grid(i, g)
        gpu_ctx.build_pyramids(ids, wins)
        first = []
        for i, g in zip(ids, grids):
            _check_levels(gpu_ctx, i, g, wins)
            first.append([gpu_ctx.download_level(i, k) for k in range(len(wins))])
        assert gpu_ctx.kernel_time("boxmax")[1] == boxmax_before + 1
        gpu_ctx.build_pyramids(ids, wins)
        for i, levels in zip(ids, first):
            for k, lv in enumerate(levels):
                assert gpu_ctx.download_level(i, k).tobytes() == lv.tobytes(), (i, k)
        assert gpu_ctx.kernel_time("boxmax")[1] == boxmax_before + 1
    finally:
        gpu_ctx.enable_kernel_timing(False)
        for i in ids:
            if gpu_ctx.has_grid(i):
                gpu_ctx.release_grid(i)


# ---------------------------------------------------------------- c. re-use of level buffers


def test_smaller_map_under_the_same_id_shows_nothing_of_the_old_level(gpu_ctx):
    full = np.full((100, 121), 65535, np.uint16)
    small = BC.make_grid(40, 71, 8, "sparse")
    gpu_ctx.upload_grid(7120, full)
    try:
        gpu_ctx.build_pyramid(7120, [1, 8])
        _check_levels(gpu_ctx, 7120, full, [1, 8])
        gpu_ctx.upload_grid(7120, small)
        gpu_ctx.build_pyramid(7120, [1, 8])
        _check_levels(gpu_ctx, 7120, small, [1, 8])
        # and through the batched entry, which keeps what exists and adds window 3
        gpu_ctx.upload_grid(7120, full)
        gpu_ctx.build_pyramids([7120], [1, 8])
        gpu_ctx.upload_grid(7120, small)
        gpu_ctx.build_pyramids([7120], [1, 8, 3])
        _check_levels(gpu_ctx, 7120, small, [1, 8, 3])
    finally:
        gpu_ctx.release_grid(7120)


def _map_local(map_pose, pose, err):
    c, s = math.cos(map_pose[2]), math.sin(map_pose[2])
    dx, dy = pose[0] + err[0] - map_pose[0], pose[1] + err[1] - map_pose[1]
    return (c * dx + s * dy, -s * dx + c * dy, pose[2] + err[2] - map_pose[2])


@pytest.mark.parametrize("kind", ["into_the_old_allocation", "past_the_old_allocation"])
def test_levels_follow_a_rebuilt_resident_map(gpu_ctx, oracle, kind):
    """construct_map_from_scans twice under one id: the second build, from fewer nodes, changes the
    base in place and its shape and pitch with it (the levels go stale and are rebuilt into their old
    buffers); from more nodes, it moves the base to a larger allocation. Either way the old levels
    are refused until a search has rebuilt them."""
    case = synth.map_case(930, n_scans=8, n_beams=360, max_range=3.0, step=0.2)
    nodes, shape0, map_pose = case["nodes"], case["shape"], case["map_pose"]
    first, second = {"into_the_old_allocation": (nodes[0:8], nodes[2:8]),
                     "past_the_old_allocation": (nodes[0:2], nodes[0:8])}[kind]
    shape1, _, _ = oracle.construct_map(shape0, map_pose, first)
    shape2, grid2, _ = oracle.construct_map(shape1, map_pose, second)
    bytes1 = shape1["rows"] * ((shape1["cols"] + 7) & ~7)
    bytes2 = shape2["rows"] * ((shape2["cols"] + 7) & ~7)
    assert max(shape2["rows"], shape2["cols"]) <= 300
    assert (bytes2 <= 1.5 * bytes1) == (kind == "into_the_old_allocation"), (shape1, shape2)
    assert (shape2["rows"], shape2["cols"]) != (shape1["rows"], shape1["cols"])
    nd = nodes[3]
    q = dict(map_id=7130, angles=nd["angles"], ranges=nd["ranges"], rel_pose=nd["rel_pose"],
             init_pose=_map_local(map_pose, nd["pose"], (0.04, -0.03, 0.01)))
    wins = [1, 2, 4, 8]
    try:
        got1, _ = gpu_ctx.construct_map_from_scans(7130, shape0, map_pose, first)
        assert got1 == shape1
        gpu_ctx.bnb_match_batch([dict(q, geom=(shape1["res"], shape1["off_x"], shape1["off_y"]))],
                                *BNB_RANGES, 3, *BNB_THRESHOLDS)
        _check_levels(gpu_ctx, 7130, gpu_ctx.download_level(7130, 0), wins)
        got2, _ = gpu_ctx.construct_map_from_scans(7130, shape1, map_pose, second)
        assert got2 == shape2
        base = gpu_ctx.download_level(7130, 0)
        assert np.array_equal(base, grid2)
        for level in (1, 2, 3):
            _refused(L.CSM_ENOENT, gpu_ctx.download_level, 7130, level)
        gpu_ctx.bnb_match_batch([dict(q, geom=(shape2["res"], shape2["off_x"], shape2["off_y"]))],
                                *BNB_RANGES, 3, *BNB_THRESHOLDS)
        _check_levels(gpu_ctx, 7130, base, wins)
    finally:
        if gpu_ctx.has_grid(7130):
            gpu_ctx.release_grid(7130)


# ---------------------------------------------------------------- d. limits


def _room(seed=40):
    """A 97 x 129 room map and a scan inside it: a search on it has a real winner."""
    case = synth.csm_case(seed, rows=97, cols=129, n_beams=360)
    q = dict(geom=case["geom"], angles=case["angles"], ranges=case["ranges"], rel_pose=case["rel_pose"],
             init_pose=case["init_pose"])
    return case, q


@pytest.mark.parametrize("rows,cols,bad_win", [(100, 121, 0), (100, 121, 65), (40, 71, 41), (40, 71, 65),
                                               (64, 64, 65)])
def test_windows_past_the_limits_are_refused_and_cost_no_level(rows, cols, bad_win):
    grid = BC.make_grid(rows, cols, 8, "random")
    ctx = api.Context(0)
    try:
        ctx.upload_grid(1, grid)
        ctx.build_pyramids([1], [1, 8, min(rows, cols, BC.MAX_WIN)])
        had = [1, 8, min(rows, cols, BC.MAX_WIN)]
        _check_levels(ctx, 1, grid, had)
        # the batched entry keeps what exists; the refused window leaves nothing behind
        _refused(L.CSM_EINVAL, ctx.build_pyramids, [1], [1, 2, bad_win])
        _check_levels(ctx, 1, grid, had)
        assert _check_levels(ctx, 1, grid, had + [2, bad_win], must_exist=False)[:3] == [0, 1, 2]
        _refused(L.CSM_ENOENT, ctx.download_level, 1, 4)
        # the single-map entry rebuilds from the base: that stays, and what is above it is a level or refused
        _refused(L.CSM_EINVAL, ctx.build_pyramid, 1, [1, 8, bad_win])
        assert _check_levels(ctx, 1, grid, [1, 8, bad_win], must_exist=False)[:1] == [0]
        ctx.build_pyramids([1], [1, 8])
        _check_levels(ctx, 1, grid, [1, 8])
    finally:
        ctx.close()


def test_search_that_needs_window_128_is_refused_and_costs_no_level(oracle):
    case, q = _room()
    ctx = api.Context(0)
    try:
        ctx.upload_grid(1, case["grid"])
        ctx.build_pyramids([1], [1, 2, 4])
        _refused(L.CSM_EINVAL, ctx.bnb_match_batch, [dict(q, map_id=1)], *BNB_RANGES, 7, *BNB_THRESHOLDS)
        wins = [1, 2, 4, 8, 16, 32, 64, 128]
        assert _check_levels(ctx, 1, case["grid"], wins, must_exist=False)[:3] == [0, 1, 2]
        out = ctx.bnb_match_batch([dict(q, map_id=1)], *BNB_RANGES, 4, *BNB_THRESHOLDS)[0]
        _check_levels(ctx, 1, case["grid"], wins[:5])
        _same_as_oracle(out, oracle.bnb(case, *BNB_RANGES, 4, *BNB_THRESHOLDS))
    finally:
        ctx.close()


# ---------------------------------------------------------------- e. a failed batched call


def _same_as_oracle(out, want):
    raw = out["raw"]
    assert want["found"] == 1               # the case has a winner to lose
    assert out["pose_found"] == want["found"], (raw, want)
    assert (raw["best_x"], raw["best_y"], raw["best_theta"]) == (want["bestX"], want["bestY"], want["bestT"]), raw
    assert raw["score"] == want["scoreMax"]


def _pyramids(ctx, ids, qs):
    ctx.build_pyramids(ids, [1, 16])


def _bnb(ctx, ids, qs):
    return ctx.bnb_match_batch(qs, *BNB_RANGES, 4, *BNB_THRESHOLDS)


def _csm(ctx, ids, qs):
    return ctx.correlative_match_batch(qs, *CSM_RANGES, 4, 0.0, 0.0)


# entry -> (call, windows of the levels it asks for in order, side of a map B too small for them)
ENTRIES = {"build_pyramids": (_pyramids, [1, 16], 8), "bnb_batch": (_bnb, [1, 2, 4, 8, 16], 8),
           "correlative_batch": (_csm, [1, 4], 3)}


@pytest.mark.parametrize("b_map", ["not_resident", "too_small"])
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_failed_batched_call_leaves_no_unbuilt_level(oracle, entry, b_map):
    """Map A's levels are collected for the call's one launch before map B fails it (B is not
    resident: CSM_ENOENT; or too small for the call's largest window: CSM_EINVAL -- 8 x 8 for window
    16, 3 x 3 for the correlative matcher's window 4). The launch never happens. A's levels must
    then be absent, never present and unwritten: the valid retry would reuse them as bounds."""
    call, wins, small = ENTRIES[entry]
    if entry == "build_pyramids":
        case, q = None, None
        grid = BC.make_grid(97, 129, 16, "random")
    else:
        case, q = _room()
        grid = case["grid"]
    a, b = 1, 2
    ctx = api.Context(0)
    try:
        ctx.upload_grid(a, grid)
        if b_map == "too_small":
            ctx.upload_grid(b, np.full((small, small), 30000, np.uint16))
        qs = None if q is None else [dict(q, map_id=a), dict(q, map_id=b)]
        _refused(L.CSM_ENOENT if b_map == "not_resident" else L.CSM_EINVAL, call, ctx, [a, b], qs)
        assert _check_levels(ctx, a, grid, wins, must_exist=False)[:1] == [0]
        _refused(L.CSM_ENOENT, ctx.download_level, a, len(wins))
        outs = call(ctx, [a], qs and qs[:1])
        _check_levels(ctx, a, grid, wins)
        if entry == "bnb_batch":
            _same_as_oracle(outs[0], oracle.bnb(case, *BNB_RANGES, 4, *BNB_THRESHOLDS))
        if entry == "correlative_batch":
            _same_as_oracle(outs[0], oracle.csm(case, *CSM_RANGES, 4))
    finally:
        ctx.close()
