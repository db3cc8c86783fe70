"""What a context derives from a resident map and keeps between calls, after the map changes
under the same id: box-max levels, the pair-row copies (xg / xgf), the phase-major copies of
the coarse-first search, the pyramid of branch and bound, the block-allocation bitmap and the
recorded HIP graphs. Each cell warms a consumer on a map (three identical calls, so a graph is
recorded), changes the map in place of the same id, calls the consumer twice more and compares
every output with `==` against a fresh map id holding the final cells, uploaded dense, and
against the oracle's matcher or the consumer's numpy reference. The final cells themselves are
first checked against the oracle's map (construct_map / update_map) or the likelihood reference.

The worlds (tests/resident_state_cases.py; tests/test_cpu_resident_state_cases.py proves that stale
state would change every cell's answer) are twelve mutations: upload_grid over the same and over
another shape, upload_grid_blocks then upload_grid, construct_map_from_scans into the old allocation
and past it, update_map_with_scan in place and with a resize, construct_maps_from_scans (two maps in
one call, both job orders: the consumers alternate), construct_global_map in parts, a likelihood
field rebuilt from a source that changed, and release_grid followed by an upload under the same id
(the allocator may hand the same pointers out again) or under the next one (the old id must then be
refused). The consumers are the seven matchers and cost functions plus peaks, volume covariance,
motion prior, pose sets and the ray check, each single and batched where both exist.

The block-allocation bitmap follows the reference's GridMap: the cost cells mark every block of
the map allocated (csm_set_block_allocation) before the change. upload_grid starts the map afresh
(a block is allocated iff it holds a known cell); construct_map_from_scans and
update_map_with_scan carry the old bitmap through Resize / Expand, and ResetValues keeps it, so the
blocks of the old map that overlap the new one stay allocated. Their fresh-id reference holds the
final cells plus the oracle's tracked bitmap (construct_map / update_map with alloc=). A rebuilt
likelihood field starts afresh like an upload: its cell runs without a given bitmap.

The second half names coarse levels by hand: score_window and its peaks / moments / prior forms, and
windows prepared for score_windows_dev, must refuse a level that is behind level 0."""
import itertools

import numpy as np
import pytest

import peaks_reference as PR
import ray_check_reference as RC
import resident_state_cases as RS
from csm_hip import _lib as L, api
from resident_state_cases import BNB, CSM, GRID, MID, MUTATIONS, world as _world

pytestmark = pytest.mark.gpu

_ids = itertools.count(1000)


# ---------------------------------------------------------------- consumers


def _with_id(qs, map_id):
    return [dict(q, map_id=map_id) for q in qs]


def _case(grid, q):
    return dict(grid=grid, geom=q["geom"], angles=q["angles"], ranges=q["ranges"], rel_pose=q["rel_pose"],
                init_pose=q["init_pose"])


def _summaries(outs):
    return [(o["pose_found"], o["raw"], o["estimated_pose"]) for o in outs]


def _csm_single(ctx, qs):
    return _summaries([ctx.correlative_match(q["map_id"], q["geom"], q["angles"], q["ranges"], q["rel_pose"],
                                             q["init_pose"], *CSM, 0.0, 0.0) for q in qs])


def _csm_oracle(oracle, grid, qs, got):
    for q, (found, raw, est) in zip(qs, got):
        lit = oracle.csm(_case(grid, q), *CSM)
        assert found == lit["found"], (raw, lit)
        assert (raw["best_x"], raw["best_y"], raw["best_theta"]) == (lit["bestX"], lit["bestY"], lit["bestT"])
        assert raw["score"] == lit["scoreMax"]
        assert est == lit["estimatedPose"]


def _csm_batch(ctx, qs):
    return _summaries(ctx.correlative_match_batch(qs, *CSM, 0.0, 0.0))


def _bnb(ctx, qs):
    return _summaries(ctx.bnb_match_batch(qs, *BNB))


def _bnb_oracle(oracle, grid, qs, got):
    for q, (found, raw, est) in zip(qs, got):
        want = oracle.bnb(_case(grid, q), *BNB)
        assert found == want["found"], (raw, want)
        assert (raw["best_x"], raw["best_y"], raw["best_theta"]) == (want["bestX"], want["bestY"], want["bestT"])
        assert raw["score"] == want["scoreMax"]
        assert est == want["estimatedPose"]


def _grid_search(ctx, qs):
    return [(o["pose_found"], o["candidates"], o["raw"], o["estimated_pose"]) for o in
            (ctx.grid_search_match(q["map_id"], q["geom"], q["angles"], q["ranges"], q["rel_pose"],
                                   q["init_pose"], *GRID) for q in qs)]


def _grid_search_oracle(oracle, grid, qs, got):
    for q, (found, cand, raw, est) in zip(qs, got):
        want = oracle.grid_search(_case(grid, q), *GRID)
        assert cand == want["evaluations"]
        assert found == want["found"]
        assert [raw["best_x"], raw["best_y"], raw["best_theta"]] == want["bestIdx"]
        assert raw["score"] == want["scoreMax"]
        assert est == want["estimatedPose"]


def _poses(qs):
    return np.array([api.host_compound(q["init_pose"], q["rel_pose"]) for q in qs])


def _plain(d):
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def _cost(ctx, qs):
    return ([_plain(o) for o in ctx.cost_covariance_batch(qs, _poses(qs), 1e4)] +
            [_plain(o) for o in ctx.linear_solver_batch(qs, 10, 1e-4, 1e-4, 1e4)])


def _cost_oracle(oracle, grid, qs, got, alloc):
    for q, p, o in zip(qs, _poses(qs), got[:len(qs)]):
        want = oracle.cost(grid, q["geom"], q["angles"], q["ranges"], p, alloc=alloc)
        assert abs(o["normalized_cost"] * len(q["angles"]) - want) <= 1e-10 * want, (o["normalized_cost"], want)
        cov = np.asarray(oracle.covariance(grid, q["geom"], q["angles"], q["ranges"], p, 1e4, alloc=alloc))
        assert np.all(np.abs(np.asarray(o["covariance"]) - cov) <= 1e-8 * np.abs(cov).max())


def _greedy(ctx, qs):
    return ([_plain(o) for o in ctx.greedy_cost_covariance_batch(qs, _poses(qs))] +
            [_plain(o) for o in ctx.hill_climbing_batch(qs)])


def _greedy_oracle(oracle, grid, qs, got):
    for q, p, o in zip(qs, _poses(qs), got[:len(qs)]):
        cost, cov = api.host_greedy_cost(grid, q["geom"], q["angles"], q["ranges"], p, covariance=True)
        assert o["normalized_cost"] == cost / len(q["angles"])
        assert o["covariance"] == cov.tolist()
    for q, o in zip(qs, got[len(qs):]):
        want = _plain(api.host_hill_climbing(grid, q["geom"], q["angles"], q["ranges"], q["rel_pose"],
                                             q["init_pose"]))
        for key in ("normalized_initial_cost", "normalized_cost", "sensor_pose", "best_sensor_pose",
                    "estimated_pose", "iterations", "refinements", "diff_translation", "diff_rotation",
                    "covariance"):
            assert o[key] == want[key], (key, o[key], want[key])


# ---- the consumers that came after the first matrix: each checked against its numpy reference
# (RS.reference: computed once per world and consumer, shared, never changed)


def _strip(o):
    """A record without its timings (the *_us fields), all the way down; arrays as lists."""
    if isinstance(o, dict):
        return {k: _strip(v) for k, v in o.items() if not k.endswith("_us")}
    if isinstance(o, (list, tuple)):
        return [_strip(v) for v in o]
    return o.tolist() if isinstance(o, np.ndarray) else o


def _scan(q):
    return (q["map_id"], q["geom"], q["angles"], q["ranges"], q["rel_pose"], q["init_pose"])


def _peaks(ctx, qs):
    single = [ctx.correlative_peaks(*_scan(q), *RS.RANGE, RS.LOW, RS.K_MAX, RS.EXCL) for q in qs]
    return _strip(single), _strip(ctx.correlative_peaks_batch(qs, *RS.RANGE, RS.LOW, RS.K_MAX, RS.EXCL))


def _check_poses(summary, record, win, q):
    best, est = PR.poses_of(record, win, q["rel_pose"])
    assert summary["pose_found"] == 1 and summary["raw"] == record
    assert summary["best_sensor_pose"] == best and summary["estimated_pose"] == est       # bit-exact doubles
    assert (summary["win_x"], summary["win_y"], summary["win_theta"]) == win["win"]
    assert summary["candidates"] == int(np.prod(win["shape"]))


def _peaks_check(ref, qs, got):
    single, batch = got
    assert single == batch
    for q, r, out in zip(qs, ref, single):
        assert r["band"] == 0 and len(r["records"]) == RS.K_MAX
        assert [o["raw"] for o in out] == r["records"]              # field by field, score bits included
        for o, rec in zip(out, r["records"]):
            _check_poses(o, rec, r["win"], q)


def _volume_cov(ctx, qs):
    single = [ctx.correlative_covariance(*_scan(q), *RS.RANGE, RS.LOW, RS.TAU) for q in qs]
    return _strip(single), _strip(ctx.correlative_covariance_batch(qs, *RS.RANGE, RS.LOW, RS.TAU))


def _volume_cov_check(ref, qs, got):
    single, batch = got
    assert single == batch
    for q, r, out in zip(qs, ref, single):
        want, win = r["summary"], r["win"]
        assert want["moments"]["best"]["found"] == 1 and want["moments"]["support"] > 1
        assert out["moments"] == want["moments"]
        assert out["mean_offset"] == want["mean_offset"]                   # bit-exact doubles
        assert out["sensor_covariance"] == want["sensor_covariance"]
        assert out["covariance"] == want["covariance"]
        _check_poses(out["summary"], want["moments"]["best"], win, q)
        assert out["summary"]["estimated_pose"] == want["estimated_pose"]


def _prior(ctx, qs):
    single = [ctx.correlative_match_prior(*_scan(q), *RS.RANGE, RS.LOW, RS.LAMBDA) for q in qs]
    return _strip(single), _strip(ctx.correlative_match_prior_batch(qs, *RS.RANGE, RS.LOW, [RS.LAMBDA] * len(qs)))


def _prior_check(ref, qs, got):
    single, batch = got
    assert single == batch
    for q, r, out in zip(qs, ref, single):
        want, win = r["prior"], r["win"]
        assert r["band"] == 0 and want["best"]["found"] == 1 and want["best"] != want["unweighted"]
        assert out["prior"] == want
        _check_poses(out["summary"], want["best"], win, q)
        assert (out["summary"]["step_x"], out["summary"]["step_y"], out["summary"]["step_theta"]) == tuple(win["steps"])


def _pose_sets(ctx, qs):
    sets = [dict(map_id=q["map_id"], geom=q["geom"], angles=q["angles"], ranges=q["ranges"], poses=RS.pose_set(q, k))
            for k, q in enumerate(qs)]
    recs, info = ctx.score_pose_sets(sets)
    assert info["poses"] == RS.N_POSES * len(qs)
    return [dict(S=r["sum_values"].astype(np.int64).tolist(), K=r["known"].astype(np.int64).tolist()) for r in recs]


def _pose_sets_check(ref, qs, got):
    assert got == ref
    assert all(max(r["K"]) > 0 for r in ref)


def _ray_check(ctx, qs):
    records, words = ctx.ray_check_batch(qs, per_beam=True, **RS.RAY)
    return [dict(record=RC.strip(r), words=w.tolist()) for r, w in zip(records, words)]


def _ray_check_check(ref, qs, got):
    assert got == ref
    assert all(r["record"]["walked"] > 0 for r in ref)


NEW_CONSUMERS = {
    "peaks": (0, _peaks, _peaks_check),
    "volume_cov": (0, _volume_cov, _volume_cov_check),
    "prior": (0, _prior, _prior_check),
    "pose_sets": (0, _pose_sets, _pose_sets_check),
    "ray_check": (0, _ray_check, _ray_check_check),
}

CONSUMERS = {
    "csm_graphs": (0, _csm_single, _csm_oracle),
    "csm_two_phase": (L.TUNE_FORCE_TWO_PHASE, _csm_single, _csm_oracle),
    "csm_batch": (0, _csm_batch, _csm_oracle),
    "bnb_batch": (0, _bnb, _bnb_oracle),
    "grid_search": (0, _grid_search, _grid_search_oracle),
    "cost_linear": (0, _cost, _cost_oracle),
    "greedy_hill_climbing": (0, _greedy, _greedy_oracle),
    **NEW_CONSUMERS,
}


@pytest.fixture(scope="module")
def refs():
    """Fresh map ids on contexts that never saw the map under test; no graphs on the reference."""
    ctxs = {0: api.Context(0, tuning_off=L.TUNE_NO_GRAPHS),
            L.TUNE_FORCE_TWO_PHASE: api.Context(0, tuning_off=L.TUNE_FORCE_TWO_PHASE | L.TUNE_NO_GRAPHS)}
    yield ctxs
    for c in ctxs.values():
        c.close()


def _refused(call):
    with pytest.raises(api.CsmError) as err:
        call()
    assert err.value.code == L.CSM_ENOENT, err.value


@pytest.mark.parametrize("consumer", list(CONSUMERS))
@pytest.mark.parametrize("mutation", MUTATIONS)
def test_derived_state_follows_the_map(oracle, refs, mutation, consumer):
    tuning, run, check = CONSUMERS[consumer]
    world = _world(mutation, oracle)
    new = consumer in NEW_CONSUMERS
    queries, warm_queries = (world["queries_new"], world["warm_new"]) if new else (world["queries"], world["warm"])
    qid = world["qid"]
    given_bitmap = consumer == "cost_linear" and not world.get("derived_alloc_only")
    ctx = api.Context(0, tuning_off=tuning)
    try:
        world["setup"](ctx)
        if given_bitmap:
            rows, cols = ctx.shapes[MID]
            ctx.set_block_allocation(MID, 4, np.ones((-(-rows // 16), -(-cols // 16)), np.uint8))
        warm = _with_id(warm_queries, MID)
        for _ in range(3):
            run(ctx, warm)
        if mutation == "batch_build":       # both job orders, spread over the consumers
            world["mutate"](ctx, reverse=list(CONSUMERS).index(consumer) % 2 == 1)
        else:
            world["mutate"](ctx)
        assert np.array_equal(ctx.download_level(qid, 0), world["grid"])
        qs = _with_id(queries, qid)
        ctx.bound_pass_stats()
        got = [run(ctx, qs) for _ in range(2)]
        if consumer == "csm_two_phase":
            assert ctx.last_search_info()["two_phase"] == 1
        if consumer in ("csm_batch", "bnb_batch"):
            assert sum(ctx.bound_pass_stats()) > 0
        if world["gone"] is not None:
            assert not ctx.has_grid(world["gone"])
            _refused(lambda: run(ctx, _with_id(queries, world["gone"])))
    finally:
        ctx.close()
    ref = refs[tuning]
    rid = next(_ids)
    ref.upload_grid(rid, world["grid"])
    try:
        if consumer == "cost_linear":
            ref.set_block_allocation(rid, 4, world["cost_alloc"])
        want = run(ref, _with_id(queries, rid))
    finally:
        ref.release_grid(rid)
    assert got[0] == want
    assert got[1] == want
    if consumer == "cost_linear":
        check(oracle, world["grid"], qs, want, world["cost_alloc"])
    elif new:
        check(RS.reference(mutation, consumer), qs, want)
    else:
        check(oracle, world["grid"], qs, want)


# ---------------------------------------------------------------- coarse levels named by the caller


def _window(ctx, win, n_points):
    wx, wy, wt = win["win"]
    return ctx.make_window(2 * wt + 1, n_points, wx, wy, RS.LOW, 1, api.host_min_known(n_points, 0.0), 0.0)


# entry -> (the call on a window, its reference out of RS.reference(kind, ..., when)[query])
ENTRIES = {
    "score_window": (lambda ctx, w, win: ctx.score_window(MID, w, win["col"], win["row"]),
                     lambda kind, when, k: RS.reference(kind, "peaks", when)[k]["records"][0]),
    "score_window_peaks": (lambda ctx, w, win: ctx.score_window_peaks(MID, w, win["col"], win["row"], RS.K_MAX,
                                                                      RS.EXCL),
                           lambda kind, when, k: RS.reference(kind, "peaks", when)[k]["records"]),
    "score_window_moments": (lambda ctx, w, win: ctx.score_window_moments(MID, w, win["col"], win["row"], RS.TAU),
                             lambda kind, when, k: RS.reference(kind, "volume_cov", when)[k]["summary"]["moments"]),
    "score_window_prior": (lambda ctx, w, win: ctx.score_window_prior(MID, w, win["col"], win["row"], RS.LAMBDA,
                                                                      win["steps"]),
                           lambda kind, when, k: RS.reference(kind, "prior", when)[k]["prior"]),
}


@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("mutation", RS.LEVEL_MUTATIONS)
def test_named_coarse_level_goes_stale(oracle, mutation, entry):
    """Pyramid [1, L], one call, the map changes, the same window with coarse_level = 1 is refused and level 0
    is what the change left; after build_pyramid the call equals the reference on the final map."""
    call, want_of = ENTRIES[entry]
    world = _world(mutation, oracle)
    n = len(world["queries_new"][0]["angles"])
    old, fresh = want_of(mutation, "before", 0), want_of(mutation, "after", 0)
    old_win, fresh_win = (RS.reference(mutation, "peaks", when)[0]["win"] for when in ("before", "after"))
    assert old != fresh and RS.reference(mutation, "peaks", "before")[0]["band"] == 0
    ctx = api.Context(0)
    try:
        world["setup"](ctx)
        ctx.build_pyramid(MID, [1, RS.LOW])
        w = _window(ctx, old_win, n)
        assert call(ctx, w, old_win) == old
        world["mutate"](ctx)
        _refused(lambda: call(ctx, w, old_win))
        _refused(lambda: ctx.download_level(MID, 1))
        assert np.array_equal(ctx.download_level(MID, 0), world["grid"])
        ctx.build_pyramid(MID, [1, RS.LOW])
        assert np.array_equal(ctx.download_level(MID, 1), oracle.boxmax(world["grid"], RS.LOW))
        assert call(ctx, _window(ctx, fresh_win, n), fresh_win) == fresh
    finally:
        ctx.close()


@pytest.mark.parametrize("mutation", RS.LEVEL_MUTATIONS)
def test_prepared_windows_never_score_the_old_map(oracle, mutation):
    """Windows prepared for score_windows_dev before the change and scored after it: the refusal, or the
    records of the same hit indices on the final cells; never the records of the old map."""
    import torch
    dev = torch.device("cuda", 0)
    world = _world(mutation, oracle)
    before = RS.reference(mutation, "peaks", "before")
    old = [r["records"][0] for r in before]
    # the same hit indices (the geometry of before the change) on the final cells
    same_hits = RS.reference_of("peaks", world["grid"], world["warm_new"])
    fresh = [r["records"][0] for r in same_hits]
    assert all(a != b for a, b in zip(old, fresh))
    ctx = api.Context(0)
    try:
        world["setup"](ctx)
        ctx.build_pyramid(MID, [1, RS.LOW])
        keep, cols, rows, windows = [], [], [], []
        for r, q in zip(before, world["warm_new"]):
            assert r["band"] == 0
            windows.append(_window(ctx, r["win"], len(q["angles"])))
            keep += [torch.from_numpy(np.ascontiguousarray(r["win"][key], np.int32)).to(dev) for key in ("col", "row")]
            cols.append(keep[-2].data_ptr())
            rows.append(keep[-1].data_ptr())
        out = torch.zeros(len(windows) * 48, dtype=torch.uint8, device=dev)
        prepared = ctx.prepare_windows([MID] * len(windows), windows, cols, rows)

        def records():
            ctx.score_windows_dev(prepared, out.data_ptr())
            ctx.synchronize()
            torch.cuda.synchronize(dev)
            raw = out.cpu().numpy().tobytes()
            recs = [api.result_to_dict(L.Result.from_buffer_copy(raw[48 * k:48 * (k + 1)]))
                    for k in range(len(windows))]
            return [dict(r, flags=r["flags"] & ~L.FLAG_PROJ_DELTA) for r in recs]

        assert records() == old
        world["mutate"](ctx)
        try:
            got = records()
        except api.CsmError as err:
            assert err.code == L.CSM_ENOENT, err
        else:
            assert got != old
            assert [g for g, r in zip(got, same_hits) if r["band"] == 0] == \
                [f for f, r in zip(fresh, same_hits) if r["band"] == 0]
        assert np.array_equal(ctx.download_level(MID, 0), world["grid"])
    finally:
        ctx.close()
