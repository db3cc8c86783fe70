"""GPU parity of the pose sets at the paths and limits their first tests leave out (cases:
tests/pose_set_cases.py, their conditions proven by tests/test_cpu_pose_sets_cases.py): k_pose_rescore with many
fixes, fixes of several sets and a second batch; k_pose_weights over three and more tiles, ties across
wavefronts and tiles, whole wavefronts and tiles of zero weights, the eligibility edge and 2^18 poses; the
32-bit S and 42-bit key at 65536 beams of 65535; the certificate far from the origin, after unwrapped
headings and at other resolutions; several sets per call with empty ones between; sequences of calls on one
context. Every comparison is exact equality with the construction or the literal restatement."""
import numpy as np
import pytest

import pose_set_cases as PC
import pose_set_reference as R
from csm_hip import _lib as L
from csm_hip import api

pytestmark = pytest.mark.gpu

MAP_ID = 9200
MARKED = L.POSE_UNCERTAIN | L.POSE_HOST_PROJECTED


class _Maps:
    """Grids uploaded for one test and released after it."""

    def __init__(self, ctx, grids, first_id=MAP_ID):
        self.ctx, self.ids = ctx, [first_id + k for k in range(len(grids))]
        self.grids = grids

    def __enter__(self):
        for mid, g in zip(self.ids, self.grids):
            self.ctx.upload_grid(mid, g)
        return self.ids

    def __exit__(self, *exc):
        for mid in self.ids:
            self.ctx.release_grid(mid)


def _set(mid, c):
    return dict(map_id=mid, geom=c["geom"], angles=c["angles"], ranges=c["ranges"], poses=c["poses"])


def _assert_literal(rec, grid, c, what=None):
    S, K = R.score_poses(grid, c["geom"], c["angles"], c["ranges"], c["poses"])
    got_s, got_k = R.records_sk(rec)
    assert np.array_equal(got_s, S) and np.array_equal(got_k, K), what
    assert not rec["reserved"].any() and set(rec["flags"].tolist()) <= {0, MARKED}, what
    return S, K


def _assert_info(info, recs, forced, spare):
    """The marked poses are the forced ones and at most `spare` others; every one of them was rescored."""
    flags = np.concatenate([r["flags"] for r in recs])
    assert info["uncertain_poses"] == int((flags != 0).sum())
    assert forced <= info["uncertain_poses"] <= forced + spare, info
    assert info["changed_poses"] <= info["uncertain_poses"] and info["host_us"] > 0.0


def _assert_update(out, c, temperature, threshold, n_out, offset):
    """The device's update of a cell-picking case against update_fast and the host restatement."""
    got_s, got_k = R.records_sk(out["records"])
    assert np.array_equal(got_s, c["S"]) and np.array_equal(got_k, c["K"])
    assert not out["records"]["flags"].any() and out["info"]["uncertain_poses"] == 0
    w, a, upd = R.update_fast(c["S"].tolist(), c["K"].tolist(), c["n_points"], temperature, threshold, n_out, offset)
    assert out["weights"].tolist() == w
    assert out["ancestors"].tolist() == a
    assert out["update"] == upd
    host = api.host_pose_set_update(out["records"], c["n_points"], temperature, threshold, n_out, offset)
    assert host[0].tolist() == w and host[1].tolist() == a and host[2] == upd
    return w, a, upd


def _update(ctx, mid, c, temperature, threshold, n_out, offset):
    out = ctx.pose_set_update(mid, c["geom"], c["angles"], c["ranges"], c["poses"], temperature, threshold, n_out,
                              offset)
    return _assert_update(out, c, temperature, threshold, n_out, offset)


# ---- rescore ----

def test_rescore_many_fixes_of_one_set(gpu_ctx):
    c = PC.many_fixes_case()
    with _Maps(gpu_ctx, [c["grid"]]) as (mid,):
        recs, info = gpu_ctx.score_pose_sets([_set(mid, c)])
    _assert_literal(recs[0], c["grid"], c)
    assert (recs[0]["flags"][list(c["forced"])] == MARKED).all()
    _assert_info(info, recs, 23, 3)


def test_rescore_fixes_of_three_sets(gpu_ctx):
    grids, sets = PC.three_sets_case()
    with _Maps(gpu_ctx, grids) as ids:
        recs, info = gpu_ctx.score_pose_sets([_set(ids[s["map"]], s) for s in sets])
    assert [r.size for r in recs] == [s["poses"].shape[0] for s in sets] and info["poses"] == 214
    forced = 0
    for k, (s, rec) in enumerate(zip(sets, recs)):
        if rec.size:
            _assert_literal(rec, grids[s["map"]], s, k)
            assert (rec["flags"][list(s["forced"])] == MARKED).all(), k
            forced += len(s["forced"])
    _assert_info(info, recs, forced, 4)                   # at most one more per non-empty set (CPU file)


def test_rescore_in_two_batches_then_a_small_call():
    c = PC.two_batches_case()
    small = R.sweep_case(65, 257)
    small_grid = R.make_map(1)
    before = api.debug_live_bytes()
    ctx = api.Context(0)
    try:
        ctx.enable_kernel_timing()
        ctx.upload_grid(MAP_ID, c["grid"])
        ctx.upload_grid(MAP_ID + 1, small_grid)
        recs, info = ctx.score_pose_sets([_set(MAP_ID, c)])
        assert ctx.kernel_time("pose_rescore")[1] == 2   # 128 poses, then 1
        S, K = _assert_literal(recs[0], c["grid"], c)
        assert K.min() > 30000 and (recs[0]["flags"] == MARKED).all()    # every beam inside, 0.6 of the cells known
        assert info["uncertain_poses"] == 129
        recs, info = ctx.score_pose_sets([_set(MAP_ID + 1, small)])       # re-grown ps_pin / ps_fix, a stale list
        _assert_literal(recs[0], small_grid, small)
        assert info["uncertain_poses"] <= 2 and info["uncertain_poses"] == int((recs[0]["flags"] != 0).sum())
        assert ctx.kernel_time("pose_rescore")[1] == 2 + (1 if info["uncertain_poses"] else 0)
        assert api.debug_live_bytes() != before
    finally:
        ctx.close()
    assert api.debug_live_bytes() == before


# ---- weights and resampling ----

@pytest.mark.parametrize("n", PC.TILE_SHAPES)
def test_weights_tile_shapes(gpu_ctx, n):
    c = PC.tile_shape_case(n)
    with _Maps(gpu_ctx, [c["grid"]]) as (mid,):
        w, a, upd = _update(gpu_ctx, mid, c, 0.3, 0.0, n, 77 + n)
        assert upd["support"] == int((c["K"] > 0).sum()) and upd["m0"] > 1 << 32
        w, a, upd = _update(gpu_ctx, mid, c, 0.02, 0.0, 2 * n + 1, (1 << 64) - 1)
        assert 0 < upd["support"] < n


@pytest.mark.parametrize("first", PC.TIE_FIRST)
def test_weights_tie_goes_to_the_first_holder(gpu_ctx, first):
    c = PC.tie_case(first)
    with _Maps(gpu_ctx, [c["grid"]]) as (mid,):
        w, a, upd = _update(gpu_ctx, mid, c, 0.3, 0.0, PC.TIE_N, 5)
    assert upd["best_index"] == first and upd["key_max"] == R.key(60000, 1) and upd["support"] == PC.TIE_N


@pytest.mark.parametrize("layout", sorted(PC.ZERO_LAYOUTS))
def test_weights_runs_of_zeros(gpu_ctx, layout):
    c = PC.zero_runs_case(layout)
    weighted = set(c["weighted"].tolist())
    with _Maps(gpu_ctx, [c["grid"]]) as (mid,):
        for n_out in (1, 7, 4 * PC.ZERO_N):
            for offset in (0, (1 << 64) - 1, 0x123456789ABCDEF):
                w, a, upd = _update(gpu_ctx, mid, c, PC.ZERO_TEMPERATURE, 0.0, n_out, offset)
                assert set(np.nonzero(w)[0].tolist()) == weighted and upd["support"] == len(weighted)
                assert set(a) <= weighted and upd["best_index"] == min(weighted)


@pytest.mark.parametrize("threshold, need", PC.ELIGIBILITY_THRESHOLDS)
def test_weights_eligibility_edge(gpu_ctx, threshold, need):
    c = PC.eligibility_case()
    with _Maps(gpu_ctx, [c["grid"]]) as (mid,):
        w, a, upd = _update(gpu_ctx, mid, c, 0.05, threshold, 45, 11)
    eligible = c["K"] >= need
    assert upd["found"] == int(eligible.any())
    assert not np.asarray(w)[~eligible].any()
    if upd["found"]:
        keys = np.array([R.key(s, k) for s, k in zip(c["S"], c["K"])])
        assert upd["key_max"] == keys[eligible].max() and eligible[upd["best_index"]]
        assert (keys.max() > upd["key_max"]) == (need > 4)               # the K = 4 poses hold the greatest key
        assert np.asarray(w)[c["K"] == need].any()                       # K = min_known exactly is eligible
    else:
        assert a == [-1] * 45


@pytest.mark.parametrize("unique_last, offset", [(False, (1 << 64) - 1), (False, 0), (True, 3)])
def test_weights_at_the_limit_of_poses_and_outputs(gpu_ctx, unique_last, offset):
    n = PC.MAX_POSES
    c = PC.limit_case(unique_last)
    with _Maps(gpu_ctx, [c["grid"]]) as (mid,):
        w, a, upd = _update(gpu_ctx, mid, c, 0.05, 0.0, n, offset)
    if unique_last:
        assert upd["best_index"] == n - 1 and w[-1] == 1 << 24
    else:
        assert set(w) == {1 << 24} and upd["m0"] == 1 << 42 and upd["support"] == n and upd["best_index"] == 0
        assert a == list(range(n))                       # T_j = j 2^24 + (2^24 - 1 or 0)


def test_weights_beyond_the_limit_are_refused(gpu_ctx):
    c = PC.tile_shape_case(1023)
    over = np.repeat(c["poses"][:1], PC.MAX_POSES + 1, axis=0)
    with _Maps(gpu_ctx, [c["grid"]]) as (mid,):
        for poses, n_out in ((c["poses"], PC.MAX_POSES + 1), (over, 4)):
            with pytest.raises(api.CsmError) as e:
                gpu_ctx.pose_set_update(mid, c["geom"], c["angles"], c["ranges"], poses, 0.05, 0.0, n_out)
            assert e.value.code == L.CSM_EINVAL
        _update(gpu_ctx, mid, c, 0.3, 0.0, 1023, 1)      # the context still works


# ---- accumulator limits ----

def test_accumulators_at_65536_beams_of_65535(gpu_ctx):
    c = PC.accumulator_case()
    c7 = dict(c, poses=c["poses7"])
    with _Maps(gpu_ctx, [c["grid"], c["grid_low"]]) as (full, low):
        recs, info = gpu_ctx.score_pose_sets([_set(full, c)])
        assert recs[0]["sum_values"].tolist() == [PC.FULL_S] * 6 and recs[0]["known"].tolist() == [PC.FULL_K] * 6
        _assert_literal(recs[0], c["grid"], c)
        assert info["uncertain_poses"] == 0
        out = gpu_ctx.pose_set_update(low, c["geom"], c["angles"], c["ranges"], c["poses7"], PC.ACC_TEMPERATURE, 0.5, 9,
                                      12345)
        S, K = _assert_literal(out["records"], c["grid_low"], c7)
        assert S[:6].tolist() == [PC.FULL_S] * 6 and S[6] < PC.FULL_S and K[6] == PC.FULL_K
        w, a, upd = R.update_fast(S.tolist(), K.tolist(), 65536, PC.ACC_TEMPERATURE, 0.5, 9, 12345)
        assert out["weights"].tolist() == w and out["ancestors"].tolist() == a and out["update"] == upd
        assert upd["key_max"] == R.key(PC.FULL_S, PC.FULL_K) and w[6] != w[0]
        score, rate = api.host_score_from_sums(out["records"]["sum_values"][6], out["records"]["known"][6], 65536)
        assert np.isfinite(score) and score <= 1.0

        a, r = R.make_scan(1, 65537)                     # refused before anything runs; the next call is exact
        with pytest.raises(api.CsmError) as e:
            gpu_ctx.score_pose_sets([_set(full, c), dict(_set(full, c), angles=a, ranges=r)])
        assert e.value.code == L.CSM_EINVAL
        recs, _ = gpu_ctx.score_pose_sets([_set(low, c7)])
        assert np.array_equal(recs[0], out["records"])


# ---- frames and headings ----

FRAMES = PC.frame_cases()


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_frames_and_headings(gpu_ctx, name):
    c = FRAMES[name]
    with _Maps(gpu_ctx, [c["grid"]]) as (mid,):
        recs, info = gpu_ctx.score_pose_sets([_set(mid, c)])
    S, K = _assert_literal(recs[0], c["grid"], c, name)
    assert K.max() > 0
    assert info["uncertain_poses"] <= 257 // 100 and info["uncertain_poses"] == int((recs[0]["flags"] != 0).sum())


# ---- set layout ----

@pytest.mark.parametrize("group_poses", sorted(PC.LAYOUTS))
def test_layout_of_many_sets(gpu_ctx, group_poses):
    grids, sets = PC.layout_case(group_poses)
    sizes = list(PC.LAYOUTS[group_poses])
    with _Maps(gpu_ctx, grids) as ids:
        recs, info = gpu_ctx.score_pose_sets([_set(ids[s["map"]], s) for s in sets])
    assert [r.size for r in recs] == sizes and info["poses"] == sum(sizes)
    assert info["uncertain_poses"] <= sum(sizes) // 100
    for k, (s, rec) in enumerate(zip(sets, recs)):
        if rec.size:
            _assert_literal(rec, grids[s["map"]], s, k)


# ---- sequences on one context ----

def _same(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a if k not in ("info",))
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b)


def test_sequence_of_calls_equals_fresh_contexts():
    grid = R.make_map(1)
    large = R.sweep_case(5, 33001)
    seventy = R.sweep_case(360, 70)
    fixes = PC.many_fixes_case()

    def score(c, mid):
        return lambda ctx: ctx.score_pose_sets([_set(mid, c)])[0]

    def update(ctx):
        return ctx.pose_set_update(MAP_ID, seventy["geom"], seventy["angles"], seventy["ranges"], seventy["poses"],
                                   0.02, 0.1, 111, 0x123456789ABCDEF)

    def empty(ctx):
        recs, info = ctx.score_pose_sets([_set(MAP_ID, dict(large, poses=np.zeros((0, 3))))])
        assert info["poses"] == 0
        return recs

    calls = [score(large, MAP_ID), update, score(fixes, MAP_ID + 1), update, empty, score(large, MAP_ID)]

    def context():
        ctx = api.Context(0)
        ctx.upload_grid(MAP_ID, grid)
        ctx.upload_grid(MAP_ID + 1, fixes["grid"])
        return ctx

    one = context()
    try:
        got = [call(one) for call in calls]
    finally:
        one.close()
    for k, call in enumerate(calls):
        fresh = context()
        try:
            want = call(fresh)
        finally:
            fresh.close()
        assert _same(got[k], want), k
    assert (got[2][0]["flags"][list(fixes["forced"])] == MARKED).all()
    assert got[1]["update"]["found"] == 1 and got[0][0]["known"].max() > 0
