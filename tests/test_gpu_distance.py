"""GPU parity of the distance fields (csm_distance_transform, csm_build_distance_map, csm_build_distance_maps)
against tests/distance_reference.py. Bar: equality of bytes, integers and double bits; nothing has a tolerance.
Cells: d2, nearest and the downloaded field equal the reference. State: every matcher record on the field
built on the device equals the record on a second id filled by upload_grid(reference field)."""
import numpy as np
import pytest

import distance_reference as DR
from csm_hip import _lib as Lb, api, synth
from test_gpu_likelihood import _records, _strip
from test_gpu_peaks import RANGE

pytestmark = pytest.mark.gpu

SRC, DST, REF = 8500, 8501, 8502            # 8500 .. 8599: this file's ids on gpu_ctx
LONG_ROW, LONG_COL = 8503, 8504


@pytest.mark.parametrize("name,occupied_min", DR.CASES)
def test_transform_equals_the_definition(gpu_ctx, name, occupied_min):
    g, d2, nearest = DR.expected(name, occupied_min)
    gpu_ctx.upload_grid(SRC, g)
    try:
        got_d2, got_nearest = gpu_ctx.distance_transform(SRC, occupied_min)
        only_d2 = gpu_ctx.distance_transform(SRC, occupied_min, want_nearest=False)
        only_nearest = gpu_ctx.distance_transform(SRC, occupied_min, want_d2=False)
        assert np.array_equal(gpu_ctx.download_level(SRC, 0), g)            # the source is not touched
    finally:
        gpu_ctx.release_grid(SRC)
    assert np.array_equal(got_d2, d2), np.argwhere(got_d2 != d2)[:8]
    assert np.array_equal(got_nearest, nearest), np.argwhere(got_nearest != nearest)[:8]
    assert only_d2[1] is None and np.array_equal(only_d2[0], d2)
    assert only_nearest[0] is None and np.array_equal(only_nearest[1], nearest)


@pytest.mark.parametrize("keep_unknown", [False, True])
@pytest.mark.parametrize("name,R,kind,occupied_min", DR.FIELD_CASES)
def test_cells_equal_the_reference(gpu_ctx, name, R, kind, occupied_min, keep_unknown):
    g, t, want = DR.field_expected(name, R, kind, occupied_min, keep_unknown)
    gpu_ctx.upload_grid(SRC, g)
    try:
        gpu_ctx.build_distance_map(SRC, DST, radius=R, occupied_min=occupied_min, keep_unknown=keep_unknown, table=t)
        got = gpu_ctx.download_level(DST, 0)
        known = gpu_ctx.debug_grid_known(DST)
        assert np.array_equal(gpu_ctx.download_level(SRC, 0), g)            # the source is not touched
    finally:
        for m in (SRC, DST):
            if gpu_ctx.has_grid(m):
                gpu_ctx.release_grid(m)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    assert known == DR.first_known(want)


def test_no_obstacle_gives_the_last_entry_everywhere(gpu_ctx):
    g = DR.grid_of("no_obstacle")
    t = DR.table_of("ramp", 5)
    gpu_ctx.upload_grid(SRC, g)
    try:
        gpu_ctx.build_distance_map(SRC, DST, radius=5, table=t)
        assert (gpu_ctx.download_level(DST, 0) == t[25]).all()
    finally:
        for m in (SRC, DST):
            gpu_ctx.release_grid(m)


@pytest.mark.parametrize("sigma", [0.25, 0.5, 1.0])
@pytest.mark.parametrize("seed", [0, 3, 5])
def test_state_equals_an_upload_of_the_reference(gpu_ctx, seed, sigma):
    """sigma = 0.5 m and 1.0 m need R = 30 and 60: beyond what a likelihood field can be built at. The host
    reference for these 400 x 400 maps is csm_host_distance_map, proved against numpy on the small cases."""
    L = 4
    case = synth.csm_case(seed)
    res = case["geom"][0]
    R = DR.radius(sigma, res)
    assert R == round(3 * sigma / res) and (R > 16 or sigma == 0.25)
    want = api.host_distance_map(case["grid"], sigma, res)
    assert np.array_equal(want, DR.kernel(sigma, res, R)[np.minimum(api.host_distance_transform(case["grid"])[0], R * R)])
    gpu_ctx.upload_grid(SRC, case["grid"])
    gpu_ctx.build_distance_map(SRC, DST, sigma, res)                     # radius and table from sigma
    gpu_ctx.upload_grid(REF, want)
    try:
        assert np.array_equal(gpu_ctx.download_level(DST, 0), want)
        assert gpu_ctx.debug_grid_known(DST) == gpu_ctx.debug_grid_known(REF) == (0, 0)
        got, ref = _records(gpu_ctx, DST, case, L), _records(gpu_ctx, REF, case, L)
        assert got == ref
        assert got["match"]["pose_found"] == 1
        # the field is not the occupancy map: the search sees another surface
        assert got["match"]["raw"] != _strip(gpu_ctx.correlative_match(
            SRC, case["geom"], case["angles"], case["ranges"], case["rel_pose"], case["init_pose"], *RANGE, L))["raw"]
    finally:
        for m in (SRC, DST, REF):
            gpu_ctx.release_grid(m)


# the tallest (200 x 1) and the widest (1 x 200) are different maps and neither first nor last
BATCH = ["random37x53_0.03", "line200x1", "cross", "random65x130_0.002", "line1x200", "pad70", "one_cell",
         "random97x131_0.5"]


def test_batch_of_eight_shapes_equals_eight_single_calls(gpu_ctx):
    srcs, dsts, singles = [8510 + i for i in range(8)], [8520 + i for i in range(8)], [8530 + i for i in range(8)]
    t = DR.table_of("ramp", 16)
    want = [DR.field_expected(name, 16, "ramp", 32768, False)[2] for name in BATCH]
    shapes = [w.shape for w in want]
    assert max(shapes) == (200, 1) and max(shapes, key=lambda s: s[1]) == (1, 200)
    for s, name in zip(srcs, BATCH):
        gpu_ctx.upload_grid(s, DR.grid_of(name))
    try:
        gpu_ctx.build_distance_maps(srcs, dsts, radius=16, table=t)
        for s, d in zip(srcs, singles):
            gpu_ctx.build_distance_map(s, d, radius=16, table=t)
        for w, d, one in zip(want, dsts, singles):
            cells = gpu_ctx.download_level(d, 0)
            assert np.array_equal(cells, gpu_ctx.download_level(one, 0))
            assert np.array_equal(cells, w)
            assert gpu_ctx.debug_grid_known(d) == gpu_ctx.debug_grid_known(one) == DR.first_known(w)
        # the reversed list into the same destinations: every id changes its shape
        gpu_ctx.build_distance_maps(srcs[::-1], dsts, radius=16, table=t)
        for w, d in zip(want[::-1], dsts):
            assert np.array_equal(gpu_ctx.download_level(d, 0), w)
            assert gpu_ctx.debug_grid_known(d) == DR.first_known(w)
        # one source may feed several fields
        gpu_ctx.build_distance_maps([srcs[1], srcs[1]], [dsts[0], dsts[2]], radius=16, table=t)
        assert np.array_equal(gpu_ctx.download_level(dsts[0], 0), want[1])
        assert np.array_equal(gpu_ctx.download_level(dsts[2], 0), want[1])
    finally:
        for m in srcs + dsts + singles:
            if gpu_ctx.has_grid(m):
                gpu_ctx.release_grid(m)


def test_refused_calls_leave_the_destination_as_it_was(gpu_ctx):
    case = synth.csm_case(1, rows=200, cols=200)
    other = DR.grid_of("random37x53_0.03")
    t = DR.table_of("gauss", 3)
    gpu_ctx.upload_grid(SRC, case["grid"])
    gpu_ctx.upload_grid(REF, other)
    gpu_ctx.build_distance_map(SRC, DST, radius=3, table=t)
    match = lambda: _strip(gpu_ctx.correlative_match(DST, case["geom"], case["angles"], case["ranges"],
                                                     case["rel_pose"], case["init_pose"], *RANGE, 4))
    cells, record = gpu_ctx.download_level(DST, 0), match()
    over = t.copy()
    over[9] = 65535
    missing = 8599
    build, builds = gpu_ctx.build_distance_map, gpu_ctx.build_distance_maps
    # one cell past the largest side, each way: a row offset would leave int16 and d2 the key's 31 bits
    long_row, long_col = np.full((1, 32768), 700, np.uint16), np.full((32768, 1), 700, np.uint16)
    long_row[0, 5] = long_col[5, 0] = 50000
    gpu_ctx.upload_grid(LONG_ROW, long_row)
    gpu_ctx.upload_grid(LONG_COL, long_col)
    refused = [
        (Lb.CSM_EINVAL, lambda: build(LONG_ROW, DST, radius=3, table=t)),
        (Lb.CSM_EINVAL, lambda: build(LONG_COL, DST, radius=3, table=t)),
        (Lb.CSM_EINVAL, lambda: builds([REF, LONG_ROW], [DST, missing], radius=3, table=t)),
        (Lb.CSM_EINVAL, lambda: builds([LONG_COL, REF], [missing, DST], radius=3, table=t)),
        (Lb.CSM_EINVAL, lambda: gpu_ctx.distance_transform(LONG_ROW)),
        (Lb.CSM_EINVAL, lambda: gpu_ctx.distance_transform(LONG_COL)),
        (Lb.CSM_EINVAL, lambda: build(DST, DST, radius=3, table=t)),
        (Lb.CSM_EINVAL, lambda: builds([SRC, REF], [DST, DST], radius=3, table=t)),
        (Lb.CSM_EINVAL, lambda: builds([SRC, DST], [DST, missing], radius=3, table=t)),
        (Lb.CSM_EINVAL, lambda: builds([REF, SRC], [DST, REF], radius=3, table=t)),
        (Lb.CSM_ENOENT, lambda: build(missing, DST, radius=3, table=t)),
        (Lb.CSM_ENOENT, lambda: builds([REF, missing], [DST, missing + 1], radius=3, table=t)),
        (Lb.CSM_EINVAL, lambda: build(REF, DST, radius=0, table=t)),
        (Lb.CSM_EINVAL, lambda: build(REF, DST, radius=256, table=np.zeros(256 * 256 + 1, np.uint16))),
        (Lb.CSM_EINVAL, lambda: build(REF, DST, radius=3, table=over)),
        (Lb.CSM_EINVAL, lambda: build(REF, DST, radius=3, table=t, occupied_min=0)),
        (Lb.CSM_EINVAL, lambda: gpu_ctx.distance_transform(DST, 0)),
        (Lb.CSM_EINVAL, lambda: gpu_ctx.distance_transform(DST, want_d2=False, want_nearest=False)),
        (Lb.CSM_ENOENT, lambda: gpu_ctx.distance_transform(missing)),
    ]
    # no table at all: through the C entry, which the Python layer never calls without one
    no_table = Lb.DistanceParams(3, 32768, 0, 0, None)
    try:
        live = api.debug_live_bytes()
        for code, call in refused:
            with pytest.raises(api.CsmError) as err:
                call()
            assert err.value.code == code and str(err.value)
            assert not gpu_ctx.has_grid(missing) and not gpu_ctx.has_grid(missing + 1)
            assert np.array_equal(gpu_ctx.download_level(DST, 0), cells)
            assert match() == record
        assert gpu_ctx.lib.csm_build_distance_map(gpu_ctx._ctx, REF, DST, no_table) == Lb.CSM_EINVAL
        assert np.array_equal(gpu_ctx.download_level(DST, 0), cells)
        assert api.debug_live_bytes() == live
        assert np.array_equal(gpu_ctx.download_level(REF, 0), other)
        assert np.array_equal(gpu_ctx.download_level(LONG_ROW, 0), long_row)
        assert np.array_equal(gpu_ctx.download_level(LONG_COL, 0), long_col)
    finally:
        for m in (SRC, DST, REF, LONG_ROW, LONG_COL):
            if gpu_ctx.has_grid(m):
                gpu_ctx.release_grid(m)


def test_transform_leaves_the_map_and_its_levels_as_they_were(gpu_ctx):
    case = synth.csm_case(0)
    scan = (case["geom"], case["angles"], case["ranges"], case["rel_pose"], case["init_pose"])
    gpu_ctx.upload_grid(SRC, case["grid"])
    try:
        gpu_ctx.build_pyramid(SRC, [1, 4])
        before = _strip(gpu_ctx.correlative_match(SRC, *scan, *RANGE, 4))
        level = gpu_ctx.download_level(SRC, 1)
        live = api.debug_live_bytes()
        gpu_ctx.distance_transform(SRC)                      # the first call allocates the workspaces
        grown = api.debug_live_bytes()
        d2, nearest = gpu_ctx.distance_transform(SRC)
        assert api.debug_live_bytes() == grown and grown[0] >= live[0]
        want = api.host_distance_transform(case["grid"])
        assert np.array_equal(d2, want[0]) and np.array_equal(nearest, want[1])
        assert np.array_equal(gpu_ctx.download_level(SRC, 0), case["grid"])
        assert np.array_equal(gpu_ctx.download_level(SRC, 1), level)
        assert _strip(gpu_ctx.correlative_match(SRC, *scan, *RANGE, 4)) == before
    finally:
        gpu_ctx.release_grid(SRC)


def test_kernel_timers_name_the_two_passes(gpu_ctx):
    g = DR.grid_of("random65x130_0.03")
    gpu_ctx.upload_grid(SRC, g)
    try:
        gpu_ctx.enable_kernel_timing(1)
        gpu_ctx.reset_kernel_timing()
        gpu_ctx.build_distance_map(SRC, DST, radius=5, table=DR.table_of("gauss", 5))
        for name in ("distance_columns", "distance_rows"):
            ms, launches = gpu_ctx.kernel_time(name)
            assert launches == 1 and ms > 0.0
    finally:
        gpu_ctx.enable_kernel_timing(0)
        for m in (SRC, DST):
            if gpu_ctx.has_grid(m):
                gpu_ctx.release_grid(m)


def test_python_adapter_searches_the_field_and_costs_the_map(gpu_ctx):
    L = 4
    case = synth.csm_case(0)
    args = (case["grid"], case["geom"], case["angles"], case["ranges"], case["rel_pose"], case["init_pose"])
    scan = args[1:]
    M = api.ScanMatcherCorrelativeHIP
    assert M.DISTANCE_ID_BIT == 1 << 62
    with pytest.raises(api.CsmError) as err:
        M("both", L, *RANGE, ctx=gpu_ctx, likelihood_sigma=0.1, distance_sigma=0.5)
    assert err.value.code == Lb.CSM_EINVAL
    plain = M("plain", L, *RANGE, ctx=gpu_ctx)
    field = M("field", L, *RANGE, ctx=gpu_ctx, distance_sigma=0.5, distance_radius=40)
    before = _strip(plain.optimize_pose(*args))
    out = _strip(field.optimize_pose(*args, map_id=SRC))
    fid = SRC | M.DISTANCE_ID_BIT
    assert fid == M.field_id(SRC, M.DISTANCE_ID_BIT)
    try:
        assert gpu_ctx.has_grid(fid)
        # by hand: build, search on the field, cost / covariance / refinement on the occupancy map
        gpu_ctx.build_distance_map(SRC, DST, 0.5, case["geom"][0], 40)
        m = gpu_ctx.correlative_match(DST, *scan, *RANGE, L)
        q = [dict(map_id=SRC, geom=case["geom"], angles=case["angles"], ranges=case["ranges"],
                  rel_pose=case["rel_pose"], init_pose=m["estimated_pose"])]
        hand = dict(m, cost=gpu_ctx.cost_covariance_batch(q, [m["best_sensor_pose"]], 1e4)[0],
                    refined=gpu_ctx.linear_solver_batch(q, covariance_scale=1e4)[0])
        assert out == _strip(hand)
        cells = gpu_ctx.download_level(fid, 0)
        assert np.array_equal(cells, gpu_ctx.download_level(DST, 0))
        assert np.array_equal(cells, api.host_distance_map(case["grid"], 0.5, case["geom"][0], 40))
        assert out["raw"] != before["raw"]
        # a second call finds map and field resident; a throw-away map leaves neither id behind
        assert _strip(field.optimize_pose(None, *scan, map_id=SRC)) == out
        # ... under the ids this matcher uses: its nonce carries bit 62 already, so the field lies under bit 63
        nonce = field._nonce
        nonce_field = M.field_id(nonce, M.DISTANCE_ID_BIT)
        assert nonce & M.DISTANCE_ID_BIT and nonce_field == nonce | M.LIKELIHOOD_ID_BIT != nonce
        seen = []
        release = gpu_ctx.release_grid
        gpu_ctx.release_grid = lambda m: (seen.append((m, gpu_ctx.has_grid(m))), release(m))[1]
        try:
            assert _strip(field.optimize_pose(*args)) == out
        finally:
            del gpu_ctx.release_grid
        assert seen == [(nonce, True), (nonce_field, True)]         # both were resident during the call
        assert not gpu_ctx.has_grid(nonce) and not gpu_ctx.has_grid(nonce_field)
        # without the option nothing changes
        assert _strip(plain.optimize_pose(*args)) == before and "cost" not in before
    finally:
        for mid in (SRC, DST, fid):
            if gpu_ctx.has_grid(mid):
                gpu_ctx.release_grid(mid)
