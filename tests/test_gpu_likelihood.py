"""GPU parity of the likelihood-field maps (csm_build_likelihood_map, csm_build_likelihood_maps) against
tests/likelihood_reference.py. Bar: equality of bytes, integers and double bits; nothing has a tolerance.
Cells: the downloaded field equals the reference. State: every matcher record on the field built on the
device equals the record on a second id filled by upload_grid(reference output)."""
import math

import numpy as np
import pytest

import likelihood_reference as LR
from csm_hip import _lib as Lb, api, synth
from test_gpu_peaks import CASES, RANGE

pytestmark = pytest.mark.gpu

SRC, DST, REF = 8100, 8101, 8102
BNB = (2.5, 2.5, 0.5, 2, 0.3, 0.5)
LAMBDA = [[3.0, 1.0, 4.0], [1.0, 2.0, -3.0], [4.0, -3.0, 60.0]]


def _strip(o):
    """A record without its timings (the *_us fields), all the way down."""
    if isinstance(o, dict):
        return {k: _strip(v) for k, v in o.items() if not k.endswith("_us")}
    if isinstance(o, (list, tuple)):
        return [_strip(v) for v in o]
    return o.tolist() if isinstance(o, np.ndarray) else o


def _records(ctx, map_id, case, L):
    """The six calls the issue names, on map_id."""
    scan = (case["geom"], case["angles"], case["ranges"], case["rel_pose"], case["init_pose"])
    q = [dict(map_id=map_id, geom=case["geom"], angles=case["angles"], ranges=case["ranges"],
              rel_pose=case["rel_pose"], init_pose=case["init_pose"])]
    m = ctx.correlative_match(map_id, *scan, *RANGE, L)
    return _strip(dict(
        match=m,
        peaks=ctx.correlative_peaks(map_id, *scan, *RANGE, L, 4, (3, 3, 2)),
        covariance=ctx.correlative_covariance(map_id, *scan, *RANGE, L, 0.02),
        prior=ctx.correlative_match_prior(map_id, *scan, *RANGE, L, LAMBDA),
        bnb=ctx.bnb_match_batch(q, *BNB),
        cost=ctx.cost_covariance_batch(q, [m["best_sensor_pose"]], 1e4)))


@pytest.mark.parametrize("keep_unknown", [False, True])
@pytest.mark.parametrize("name,R", LR.CPU_CASES + LR.GPU_EXTRA_CASES)
def test_cells_equal_the_reference(gpu_ctx, name, R, keep_unknown):
    g, t, want = LR.expected(name, R, keep_unknown)
    gpu_ctx.upload_grid(SRC, g)
    gpu_ctx.build_likelihood_map(SRC, DST, radius=R, occupied_min=LR.occupied_min_of(name),
                                 keep_unknown=keep_unknown, kernel=t)
    got = gpu_ctx.download_level(DST, 0)
    assert np.array_equal(gpu_ctx.download_level(SRC, 0), g)            # the source is not touched
    gpu_ctx.release_grid(SRC)
    gpu_ctx.release_grid(DST)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]


def test_the_cases_reach_both_paths_of_the_kernel():
    """The kernel walks its obstacle list while a tile's halo holds at most (2R + 1)^2 obstacles and visits
    the taps of the disc beyond that: dense64 at R = 16 is past the switch in both of its tiles (rows 0..47
    and 16..63 with their halos), the seams grid is below it at R = 3 and R = 16."""
    g = LR.grid_of("dense64") >= 32768
    assert int(g[:48].sum()) > 33 * 33 and int(g[16:].sum()) > 33 * 33
    assert int((LR.grid_of("seams") >= 32768).sum()) < 7 * 7


@pytest.mark.parametrize("seed,L,sigma", [CASES[0] + (0.05,), CASES[3] + (0.1,), CASES[5] + (0.25,)])
def test_state_equals_an_upload_of_the_reference(gpu_ctx, seed, L, sigma):
    case = synth.csm_case(seed)
    res = case["geom"][0]
    R = LR.radius(sigma, res)
    want = LR.likelihood_map(case["grid"], LR.kernel(sigma, res, R), R)
    assert (want != case["grid"]).sum() > 3000
    gpu_ctx.upload_grid(SRC, case["grid"])
    gpu_ctx.build_likelihood_map(SRC, DST, sigma, res)                   # radius and table from sigma
    gpu_ctx.upload_grid(REF, want)
    try:
        assert np.array_equal(gpu_ctx.download_level(DST, 0), want)
        got, ref = _records(gpu_ctx, DST, case, L), _records(gpu_ctx, REF, case, L)
        assert got == ref
        assert got["match"]["pose_found"] == 1
        # the field is not the occupancy map: the search sees another surface
        assert got["match"]["raw"] != _strip(gpu_ctx.correlative_match(
            SRC, case["geom"], case["angles"], case["ranges"], case["rel_pose"], case["init_pose"], *RANGE, L))["raw"]
    finally:
        for m in (SRC, DST, REF):
            gpu_ctx.release_grid(m)


SHAPES = ["random16", "random37x53", "random65x130", "seams", "dense64"]


def test_batch_of_five_shapes_equals_five_single_calls(gpu_ctx):
    srcs, dsts, singles = [8200 + i for i in range(5)], [8210 + i for i in range(5)], [8220 + i for i in range(5)]
    t = LR.kernel(LR.sigma_of(3), LR.RES, 3)
    for s, name in zip(srcs, SHAPES):
        gpu_ctx.upload_grid(s, LR.grid_of(name))
    gpu_ctx.build_likelihood_maps(srcs, dsts, radius=3, kernel=t)
    for s, d in zip(srcs, singles):
        gpu_ctx.build_likelihood_map(s, d, radius=3, kernel=t)
    try:
        for name, d, one in zip(SHAPES, dsts, singles):
            cells = gpu_ctx.download_level(d, 0)
            assert np.array_equal(cells, gpu_ctx.download_level(one, 0))
            assert np.array_equal(cells, LR.expected(name, 3, False)[2])
        # one source may feed several fields
        gpu_ctx.build_likelihood_maps([srcs[1], srcs[1]], [dsts[0], dsts[2]], radius=3, kernel=t)
        assert np.array_equal(gpu_ctx.download_level(dsts[0], 0), LR.expected(SHAPES[1], 3, False)[2])
        assert np.array_equal(gpu_ctx.download_level(dsts[2], 0), LR.expected(SHAPES[1], 3, False)[2])
    finally:
        for m in srcs + dsts + singles:
            gpu_ctx.release_grid(m)


def test_refused_calls_leave_the_destination_as_it_was(gpu_ctx):
    case = synth.csm_case(1, rows=200, cols=200)
    other = LR.grid_of("random37x53")
    t = LR.kernel(0.05, 0.05, 3)
    gpu_ctx.upload_grid(SRC, case["grid"])
    gpu_ctx.upload_grid(REF, other)
    gpu_ctx.build_likelihood_map(SRC, DST, radius=3, kernel=t)
    match = lambda: _strip(gpu_ctx.correlative_match(DST, case["geom"], case["angles"], case["ranges"],
                                                     case["rel_pose"], case["init_pose"], *RANGE, 4))
    cells, record = gpu_ctx.download_level(DST, 0), match()
    over = t.copy()
    over[9] = 32769
    missing = 8199
    refused = [
        (Lb.CSM_EINVAL, lambda: gpu_ctx.build_likelihood_map(DST, DST, radius=3, kernel=t)),
        (Lb.CSM_EINVAL, lambda: gpu_ctx.build_likelihood_maps([SRC, REF], [DST, DST], radius=3, kernel=t)),
        (Lb.CSM_EINVAL, lambda: gpu_ctx.build_likelihood_maps([SRC, DST], [DST, missing], radius=3, kernel=t)),
        (Lb.CSM_EINVAL, lambda: gpu_ctx.build_likelihood_maps([REF, SRC], [DST, REF], radius=3, kernel=t)),
        (Lb.CSM_ENOENT, lambda: gpu_ctx.build_likelihood_map(missing, DST, radius=3, kernel=t)),
        (Lb.CSM_ENOENT, lambda: gpu_ctx.build_likelihood_maps([REF, missing], [DST, missing + 1], radius=3,
                                                              kernel=t)),
        (Lb.CSM_EINVAL, lambda: gpu_ctx.build_likelihood_map(REF, DST, radius=0, kernel=t)),
        (Lb.CSM_EINVAL, lambda: gpu_ctx.build_likelihood_map(REF, DST, radius=17, kernel=np.zeros(290, np.uint32))),
        (Lb.CSM_EINVAL, lambda: gpu_ctx.build_likelihood_map(REF, DST, radius=3, kernel=over)),
        (Lb.CSM_EINVAL, lambda: gpu_ctx.build_likelihood_map(REF, DST, radius=3, kernel=t, occupied_min=0)),
    ]
    try:
        for code, call in refused:
            with pytest.raises(api.CsmError) as err:
                call()
            assert err.value.code == code and str(err.value)
            assert not gpu_ctx.has_grid(missing) and not gpu_ctx.has_grid(missing + 1)
            assert np.array_equal(gpu_ctx.download_level(DST, 0), cells)
            assert match() == record
        assert np.array_equal(gpu_ctx.download_level(REF, 0), other)
    finally:
        for m in (SRC, DST, REF):
            gpu_ctx.release_grid(m)


def _map_local(map_pose, pose, err):
    c, s = math.cos(map_pose[2]), math.sin(map_pose[2])
    dx, dy = pose[0] + err[0] - map_pose[0], pose[1] + err[1] - map_pose[1]
    return (c * dx + s * dy, -s * dx + c * dy, pose[2] + err[2] - map_pose[2])


@pytest.mark.parametrize("tuning", [0, Lb.TUNE_FORCE_TWO_PHASE], ids=["graphs", "two_phase"])
def test_resident_state_follows_a_rebuilt_field(tuning):
    """A field that was matched on until its chain replays as a graph (or its phase-major copy exists) is
    rebuilt from a source that changed; the next match equals a fresh upload's. Then a rebuild into another
    shape, and no byte is left behind once both ids are released."""
    world = synth.map_case(930, n_scans=14, n_beams=1080, max_range=5.0, step=0.3)
    nodes, shape0 = world["nodes"], world["shape"]
    map_pose = nodes[0]["pose"]
    nd = nodes[6]
    small = LR.grid_of("random65x130")
    before = api.debug_live_bytes()
    ctx = api.Context(0, tuning_off=tuning)
    ref = api.Context(0, tuning_off=tuning | Lb.TUNE_NO_GRAPHS)
    after_pass = []
    try:
        for _ in range(2):
            shape1, _ = ctx.construct_map_from_scans(SRC, shape0, map_pose, nodes[0:10])
            geom = (shape1["res"], shape1["off_x"], shape1["off_y"])
            scan = (geom, nd["angles"], nd["ranges"], nd["rel_pose"], _map_local(map_pose, nd["pose"], (0.04, -0.03, 0.01)))
            match = lambda c, m: _strip(c.correlative_match(m, *scan, *RANGE, 4))
            ctx.build_likelihood_map(SRC, DST, 0.05, shape1["res"])
            # the first match builds the pair-row copy, the next three are sightings, the third of them
            # records the chain: the fifth match replays it
            first = [match(ctx, DST) for _ in range(5)]
            assert first[1:] == first[:-1]
            info = ctx.last_search_info()
            assert info["two_phase"] == (1 if tuning else 0)
            if not tuning:
                assert info["graph_replayed"] == 1
            shape2, _ = ctx.update_map_with_scan(SRC, shape1, map_pose, nodes[5])
            assert (shape2["rows"], shape2["cols"]) == (shape1["rows"], shape1["cols"])
            src_cells = ctx.download_level(SRC, 0)
            ctx.build_likelihood_map(SRC, DST, 0.1, shape1["res"])
            want = LR.likelihood_map(src_cells, LR.kernel(0.1, shape1["res"], 6), 6)
            assert LR.radius(0.1, shape1["res"]) == 6
            assert np.array_equal(ctx.download_level(DST, 0), want)
            got = [match(ctx, DST) for _ in range(2)]
            ref.upload_grid(REF, want)
            fresh = match(ref, REF)
            ref.release_grid(REF)
            assert got == [fresh, fresh]
            assert fresh != first[0]
            # another shape under the same id
            ctx.upload_grid(REF, small)
            ctx.build_likelihood_map(REF, DST, radius=3, kernel=LR.kernel(LR.sigma_of(3), LR.RES, 3))
            assert np.array_equal(ctx.download_level(DST, 0), LR.expected("random65x130", 3, False)[2])
            for m in (SRC, DST, REF):
                ctx.release_grid(m)
            after_pass.append(api.debug_live_bytes())
        assert after_pass[0] == after_pass[1]           # workspaces at their size: a pass leaves nothing behind
    finally:
        ctx.close()
        ref.close()
    assert api.debug_live_bytes() == before


def test_python_adapter_searches_the_field_and_costs_the_map(gpu_ctx):
    L = 4
    case = synth.csm_case(0)
    args = (case["grid"], case["geom"], case["angles"], case["ranges"], case["rel_pose"], case["init_pose"])
    scan = args[1:]
    plain = api.ScanMatcherCorrelativeHIP("plain", L, *RANGE, ctx=gpu_ctx)
    field = api.ScanMatcherCorrelativeHIP("field", L, *RANGE, ctx=gpu_ctx, likelihood_sigma=0.1)
    before = _strip(plain.optimize_pose(*args))
    out = _strip(field.optimize_pose(*args, map_id=SRC))
    fid = SRC | api.ScanMatcherCorrelativeHIP.LIKELIHOOD_ID_BIT
    try:
        assert gpu_ctx.has_grid(fid)
        # by hand: build, search on the field, cost / covariance / refinement on the occupancy map
        gpu_ctx.build_likelihood_map(SRC, DST, 0.1, case["geom"][0])
        m = gpu_ctx.correlative_match(DST, *scan, *RANGE, L)
        q = [dict(map_id=SRC, geom=case["geom"], angles=case["angles"], ranges=case["ranges"],
                  rel_pose=case["rel_pose"], init_pose=m["estimated_pose"])]
        hand = dict(m, cost=gpu_ctx.cost_covariance_batch(q, [m["best_sensor_pose"]], 1e4)[0],
                    refined=gpu_ctx.linear_solver_batch(q, covariance_scale=1e4)[0])
        assert out == _strip(hand)
        assert np.array_equal(gpu_ctx.download_level(fid, 0), gpu_ctx.download_level(DST, 0))
        assert out["raw"] != before["raw"]
        # a second call finds map and field resident; a throw-away map leaves neither behind
        assert _strip(field.optimize_pose(None, *scan, map_id=SRC)) == out
        assert _strip(field.optimize_pose(*args)) == out
        assert not gpu_ctx.has_grid(1 << 62) and not gpu_ctx.has_grid(1 << 62 | 1 << 63)
        # without the option nothing changes
        direct = _strip(gpu_ctx.correlative_match(SRC, *scan, *RANGE, L))
        assert before == direct and "cost" not in before
        assert _strip(plain.optimize_pose(*args)) == before
    finally:
        for mid in (SRC, DST, fid):
            if gpu_ctx.has_grid(mid):
                gpu_ctx.release_grid(mid)
