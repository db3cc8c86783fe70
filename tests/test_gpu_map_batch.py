"""GPU parity of csm_construct_maps_from_scans (many maps per call, one launch chain
per chunk) against the literal CPU builder, and its equivalence with the loop of
csm_construct_map_from_scans calls it replaces: cells, geometry, counters and every
piece of state a later call reads. Cases: tests/map_batch_cases.py (their
properties are proven in tests/test_cpu_map_batch_cases.py)."""
import math

import numpy as np
import pytest

import map_batch_cases as MB
from csm_hip import _lib as L, api

pytestmark = pytest.mark.gpu

BASE = 9000


@pytest.fixture(scope="module")
def cases():
    return MB.build()


@pytest.fixture(scope="module")
def wanted(oracle, cases):
    """The oracle's (shape, grid, stats) of every case, computed once and never changed."""
    out = {}
    for name, case in cases:
        shape, grid, stats = oracle.construct_map(case["shape"], case["map_pose"], case["nodes"])
        grid.setflags(write=False)
        out[name] = (shape, grid, stats)
    return out


def _jobs(cases, base=BASE):
    return [dict(map_id=base + i, shape=c["shape"], map_pose=c["map_pose"], nodes=c["nodes"])
            for i, (_, c) in enumerate(cases)]


def _check_one(ctx, map_id, result, want, name):
    want_shape, want_grid, stats = want
    shape, info, status = result
    assert status == 0, name
    assert shape == want_shape, name
    got = ctx.download_level(map_id, 0)
    assert got.shape == want_grid.shape, name
    bad = np.argwhere(got != want_grid)
    assert bad.size == 0, (name, len(bad), bad[:5], got[tuple(bad[0])], want_grid[tuple(bad[0])])
    assert info["rays"] == stats["rays"], name
    assert info["cell_updates"] == stats["updates"], name
    assert info["saturated_reads"] == stats["oob_reads"], name
    ys, xs = np.nonzero(want_grid)
    first = (ys.min(), xs.min()) if ys.size else want_grid.shape      # nothing known: rows / cols
    assert (info["first_known_row"], info["first_known_col"]) == first, name
    assert ctx.debug_grid_known(map_id) == tuple(first), name


def _check_all(ctx, cases, wanted, results, base=BASE):
    assert len(results) == len(cases)
    for i, (name, _) in enumerate(cases):
        _check_one(ctx, base + i, results[i], wanted[name], name)


def _release(ctx, n, base=BASE):
    for i in range(n):
        if ctx.has_grid(base + i):
            ctx.release_grid(base + i)


@pytest.mark.parametrize("name", list(MB.CASES))
def test_every_case_alone(gpu_ctx, cases, wanted, name):
    case = dict(cases)[name]
    results, binfo = gpu_ctx.construct_maps_from_scans(_jobs([(name, case)]))
    _check_all(gpu_ctx, [(name, case)], wanted, results)
    assert binfo["chunks"] == 1
    _release(gpu_ctx, 1)


@pytest.mark.parametrize("order", ["forwards", "reversed"])
def test_all_cases_in_one_call(gpu_ctx, cases, wanted, order):
    """48 x 48 next to 288 x 288 cells, 0 and 1 ray next to 21,570: one launch chain."""
    mixed = cases if order == "forwards" else cases[::-1]
    results, binfo = gpu_ctx.construct_maps_from_scans(_jobs(mixed))
    assert binfo["chunks"] == 1
    _check_all(gpu_ctx, mixed, wanted, results)
    _release(gpu_ctx, len(mixed))


def _local(map_pose, pose):
    c, s_ = math.cos(map_pose[2]), math.sin(map_pose[2])
    dx, dy = pose[0] - map_pose[0], pose[1] - map_pose[1]
    return (c * dx + s_ * dy, -s_ * dx + c * dy, pose[2] - map_pose[2])


def _queries(cases, shapes, base=BASE):
    """One query per map: its last scan from a pose a little off the true one, map-local."""
    out = []
    for i, (_, case) in enumerate(cases):
        nd, shape = case["nodes"][-1], shapes[i]
        init = _local(case["map_pose"], (nd["pose"][0] + 0.08, nd["pose"][1] - 0.06, nd["pose"][2] + 0.015))
        out.append(dict(map_id=base + i, geom=(shape["res"], shape["off_x"], shape["off_y"]), angles=nd["angles"],
                        ranges=nd["ranges"], rel_pose=nd["rel_pose"], init_pose=init))
    return out


def _match_all(ctx, queries):
    out = []
    for q in queries:
        s = ctx.correlative_match(q["map_id"], q["geom"], q["angles"], q["ranges"], q["rel_pose"], q["init_pose"],
                                  0.5, 0.5, 0.2, 4, 0.0, 0.0)
        out.append((s["pose_found"], s["estimated_pose"], s["best_sensor_pose"], s["raw"]))
    return out


def test_batch_leaves_what_the_loop_of_single_calls_leaves(cases):
    """Context A: the loop. Context B: one call. Cells, first known row / column, a match against each
    map, and the cost / covariance at the matched poses (which reads the block allocation that the
    builds carried): bit-equal."""
    a, b = api.Context(0), api.Context(0)
    try:
        jobs = _jobs(cases)
        singles = [a.construct_map_from_scans(j["map_id"], j["shape"], j["map_pose"], j["nodes"]) for j in jobs]
        results, _ = b.construct_maps_from_scans(jobs)
        for j, (shape, info), (shape_b, info_b, status) in zip(jobs, singles, results):
            assert status == 0 and shape_b == shape
            for key in ("rays", "cell_updates", "saturated_reads", "first_known_row", "first_known_col",
                        "device_projection"):
                assert info_b[key] == info[key], (j["map_id"], key)
            assert np.array_equal(a.download_level(j["map_id"], 0), b.download_level(j["map_id"], 0))
            assert a.debug_grid_known(j["map_id"]) == b.debug_grid_known(j["map_id"])
        queries = _queries(cases, [s for s, _ in singles])
        match_a, match_b = _match_all(a, queries), _match_all(b, queries)
        assert match_a == match_b
        assert sum(m[0] for m in match_a) >= len(cases) - 4      # the maps with a ray or none do not match
        poses = [m[2] for m in match_a]
        for ca, cb in zip(a.cost_covariance_batch(queries, poses, 1e4), b.cost_covariance_batch(queries, poses, 1e4)):
            assert np.array_equal(ca["normalized_cost"], cb["normalized_cost"], equal_nan=True)
            assert np.array_equal(ca["covariance"], cb["covariance"], equal_nan=True)
            assert np.array_equal(ca["hessian"], cb["hessian"], equal_nan=True)
    finally:
        a.close()
        b.close()


def test_rebuild_in_place(oracle, cases, wanted):
    """Resident maps with box-max levels and a phase-major copy are rebuilt by one call from moved
    nodes, in the frames the first build left: the cells are the oracle's and a match afterwards
    is the match on an upload of the oracle's grid (nothing stale is read)."""
    ctx, ref = api.Context(0, tuning_off=L.TUNE_FORCE_TWO_PHASE), api.Context(0, tuning_off=L.TUNE_FORCE_TWO_PHASE)
    try:
        jobs = _jobs(cases)
        results, _ = ctx.construct_maps_from_scans(jobs)
        _check_all(ctx, cases, wanted, results)
        names = [n for n, _ in cases]
        ten, odd = BASE + names.index("ten"), BASE + names.index("odd")
        ctx.build_pyramid(ten, [1, 4])
        ctx.build_pyramid(odd, [1, 4])
        q0 = _queries(cases, [r[0] for r in results])
        assert _match_all(ctx, [q0[names.index("ten")]])[0][0] == 1        # leaves a phase-major copy
        # the nodes moved (an optimization) and the window slid by one scan
        moved = []
        for i, (name, case) in enumerate(cases):
            nodes = case["nodes"][1:] if len(case["nodes"]) > 1 else case["nodes"]
            nodes = [dict(nd, pose=(nd["pose"][0] + 0.031, nd["pose"][1] - 0.017, nd["pose"][2] + 0.004))
                     for nd in nodes]
            moved.append((name, dict(case, shape=results[i][0], nodes=nodes, map_pose=nodes[0]["pose"])))
        want2 = {n: oracle.construct_map(c["shape"], c["map_pose"], c["nodes"]) for n, c in moved}
        results2, _ = ctx.construct_maps_from_scans(_jobs(moved))
        _check_all(ctx, moved, want2, results2)
        for i, (name, _) in enumerate(moved):
            ref.upload_grid(BASE + i, want2[name][1])
        q1 = _queries(moved, [r[0] for r in results2])
        assert _match_all(ctx, q1) == _match_all(ref, q1)
    finally:
        ctx.close()
        ref.close()


def test_chunks_give_the_same_bytes(gpu_ctx, cases, wanted):
    results, binfo = gpu_ctx.construct_maps_from_scans(_jobs(cases))
    assert binfo["chunks"] == 1
    whole = [gpu_ctx.download_level(BASE + i, 0) for i in range(len(cases))]
    _release(gpu_ctx, len(cases))
    for limit, chunks in ((6 << 20, None), (1, len(cases))):
        results, binfo = gpu_ctx.construct_maps_from_scans(_jobs(cases), scratch_limit_bytes=limit)
        assert binfo["chunks"] >= 3 if chunks is None else binfo["chunks"] == chunks, binfo
        _check_all(gpu_ctx, cases, wanted, results)
        for i in range(len(cases)):
            assert np.array_equal(gpu_ctx.download_level(BASE + i, 0), whole[i])
        _release(gpu_ctx, len(cases))


def test_host_projection_is_per_map(cases, wanted):
    """With room for one uncertain beam, the two maps with beams along cell edges (at least two each:
    proven in the CPU test) are projected on the host; the rest of their chunk stays on the device."""
    small = api.Context(0, map_uncertain_cap=1)
    try:
        results, binfo = small.construct_maps_from_scans(_jobs(cases))
        assert binfo["chunks"] == 1
        _check_all(small, cases, wanted, results)
        dev = {name: results[i][1]["device_projection"] for i, (name, _) in enumerate(cases)}
        assert dev["aligned"] == 0 and dev["odd"] == 0
        # no usable beam: nothing certifies that the box spreads, as in the single call
        assert dev["none_usable"] == 0 and dev["none_usable_one_node"] == 0
        for name in ("one_scan", "ten", "saturate", "tiny", "one_usable", "fine", "blocks_of_4", "blocks_of_32",
                     "shared_a", "shared_b"):
            assert dev[name] == 1, name
        assert binfo["host_projection_jobs"] == sum(1 for v in dev.values() if v == 0)
    finally:
        small.close()


def test_shared_scans_are_uploaded_once(gpu_ctx, cases, wanted):
    pair = [(n, c) for n, c in cases if n in ("shared_a", "shared_b")]
    results, binfo = gpu_ctx.construct_maps_from_scans(_jobs(pair))
    _check_all(gpu_ctx, pair, wanted, results)
    one_copy = sum(2 * 8 * len(nd["ranges"]) for nd in pair[0][1]["nodes"])
    assert binfo["scan_bytes_uploaded"] == one_copy
    # two maps over their own copies of the arrays: twice the bytes, the same maps
    own = [(pair[0][0], pair[0][1]),
           (pair[1][0], dict(pair[1][1], nodes=[dict(nd, angles=np.array(nd["angles"]), ranges=np.array(nd["ranges"]))
                                                for nd in pair[1][1]["nodes"]]))]
    results, binfo = gpu_ctx.construct_maps_from_scans(_jobs(own))
    _check_all(gpu_ctx, own, wanted, results)
    assert binfo["scan_bytes_uploaded"] == 2 * one_copy
    _release(gpu_ctx, 2)


def test_refusals(gpu_ctx, cases, wanted):
    three = [(n, c) for n, c in cases if n in ("one_scan", "tiny", "odd")]
    results, _ = gpu_ctx.construct_maps_from_scans(_jobs(three))
    before = gpu_ctx.download_level(BASE, 0)
    # whole-call refusals: nothing changes
    dup = _jobs(three)
    dup[2]["map_id"] = dup[0]["map_id"]
    with pytest.raises(api.CsmError):
        gpu_ctx.construct_maps_from_scans(dup)
    with pytest.raises(api.CsmError):
        gpu_ctx.construct_maps_from_scans(_jobs(three[::-1]), subpixel_scale=0)
    with pytest.raises(api.CsmError):
        gpu_ctx.construct_maps_from_scans(_jobs(three), scratch_limit_bytes=-1)
    with pytest.raises(api.CsmError):
        gpu_ctx.construct_maps_from_scans([])
    assert np.array_equal(gpu_ctx.download_level(BASE, 0), before)
    _check_all(gpu_ctx, three, wanted, results)
    # one job without nodes: its status says so, its map stays, the others are built
    jobs = _jobs(three[::-1])
    jobs[2] = dict(jobs[2], nodes=[])                 # map BASE + 2 holds "odd"; the job is three[0]'s
    results2, _ = gpu_ctx.construct_maps_from_scans(jobs)
    assert [r[2] for r in results2] == [0, 0, L.CSM_EINVAL]
    assert results2[2][0] == three[0][1]["shape"]     # its shape comes back as it went in
    _check_all(gpu_ctx, three[::-1][:2], wanted, results2[:2])
    odd = gpu_ctx.download_level(BASE + 2, 0)
    assert np.array_equal(odd, wanted["odd"][1])      # still the first call's map
    _release(gpu_ctx, 3)


def _refused_cases():
    """Three jobs the single call refuses only after the projection: usable beams that all point along
    +x (the box has no extent in y), a lone sensor at a positive position without a usable beam (no
    extent at all), and two sensors so far apart that the resized map would pass 2^28 cells."""
    angles, ranges = np.array([0.0, 0.0, 0.0]), np.array([2.0, 3.0, 1.5])
    shape = dict(res=0.05, off_x=0.0, off_y=0.0, rows=32, cols=32, log2_block=4)
    along_x = dict(pose=(0.3, 0.2, 0.0), angles=angles, ranges=ranges, rel_pose=(0.0, 0.0, 0.0),
                   min_range=0.0, max_range=10.0)
    blind = dict(along_x, max_range=0.02)
    far = [dict(along_x, angles=np.array([0.3, 1.1, 2.0])), dict(along_x, pose=(1000.3, 1000.2, 0.0),
                                                                  angles=np.array([0.3, 1.1, 2.0]))]
    return [("flat_box", dict(nodes=[along_x], map_pose=(0.0, 0.0, 0.0), shape=shape)),
            ("no_box", dict(nodes=[blind], map_pose=(0.0, 0.0, 0.0), shape=shape)),
            ("too_large", dict(nodes=far, map_pose=(0.0, 0.0, 0.0), shape=shape))]


@pytest.mark.parametrize("limit", [0, 1 << 40])
def test_jobs_refused_after_the_projection(gpu_ctx, oracle, cases, wanted, limit):
    """An empty bounding box and a resize out of range are found when the chunk is already on its way:
    those jobs get their status, their resident maps stay, and the other jobs of the chunk complete.
    With the default limit the too-large job's bound puts it into a chunk of its own; with a huge
    limit all jobs share one chunk."""
    refused = _refused_cases()
    for _, c in refused[:2]:                  # the reference asserts; the third is the library's own limit
        with pytest.raises(ValueError):
            oracle.construct_map(c["shape"], c["map_pose"], c["nodes"])
    good = [(n, c) for n, c in cases if n in ("ten", "tiny", "one_usable", "odd")]
    mixed = [good[0], refused[0], good[1], refused[1], refused[2], good[2], good[3]]
    bad_at = [1, 3, 4]
    old = np.arange(32 * 32, dtype=np.uint16).reshape(32, 32)
    for i in bad_at:
        gpu_ctx.upload_grid(BASE + i, old)
    results, binfo = gpu_ctx.construct_maps_from_scans(_jobs(mixed), scratch_limit_bytes=limit)
    assert binfo["chunks"] == (1 if limit else 3)
    for i, (name, case) in enumerate(mixed):
        if i in bad_at:
            assert results[i][2] == L.CSM_EINVAL, name
            assert results[i][0] == case["shape"], name
            assert np.array_equal(gpu_ctx.download_level(BASE + i, 0), old), name
        else:
            _check_one(gpu_ctx, BASE + i, results[i], wanted[name], name)
    # the single call refuses the same jobs and leaves the same maps
    for i in bad_at:
        c = mixed[i][1]
        with pytest.raises(api.CsmError):
            gpu_ctx.construct_map_from_scans(BASE + i, c["shape"], c["map_pose"], c["nodes"])
        assert np.array_equal(gpu_ctx.download_level(BASE + i, 0), old)
    _release(gpu_ctx, len(mixed))


def test_single_builds_after_a_batch(gpu_ctx, oracle, cases, wanted):
    """The batch and the single entries share their scratch buffers."""
    results, _ = gpu_ctx.construct_maps_from_scans(_jobs(cases))
    case = dict(cases)["ten"]
    shape, info = gpu_ctx.construct_map_from_scans(BASE + 100, case["shape"], case["map_pose"], case["nodes"][:6])
    want_shape, want_grid, stats = oracle.construct_map(case["shape"], case["map_pose"], case["nodes"][:6])
    assert shape == want_shape and np.array_equal(gpu_ctx.download_level(BASE + 100, 0), want_grid)
    assert info["cell_updates"] == stats["updates"]
    want_shape2, want_grid2, stats2 = oracle.update_map(want_shape, want_grid, case["map_pose"], case["nodes"][6])
    shape2, info2 = gpu_ctx.update_map_with_scan(BASE + 100, shape, case["map_pose"], case["nodes"][6])
    assert shape2 == want_shape2 and np.array_equal(gpu_ctx.download_level(BASE + 100, 0), want_grid2)
    assert (info2["rays"], info2["cell_updates"]) == (stats2["rays"], stats2["updates"])
    # and the batch again, after the single calls left their sizes in the buffers
    results, _ = gpu_ctx.construct_maps_from_scans(_jobs(cases))
    _check_all(gpu_ctx, cases, wanted, results)
    gpu_ctx.release_grid(BASE + 100)
    _release(gpu_ctx, len(cases))


def test_tables_follow_the_settings(gpu_ctx, oracle, cases):
    """Two batch calls with different probabilities: the second must not run on the first's tables
    (the hit table is loaded once per workgroup, from whatever the context holds)."""
    pick = [(n, c) for n, c in cases if n in ("ten", "tiny")]
    for kw, okw in ((dict(prob_hit=0.62, prob_miss=0.46), dict(prob_hit=0.62, prob_miss=0.46)),
                    (dict(prob_hit=0.9, prob_miss=0.1), dict(prob_hit=0.9, prob_miss=0.1))):
        results, _ = gpu_ctx.construct_maps_from_scans(_jobs(pick), **kw)
        want = {n: oracle.construct_map(c["shape"], c["map_pose"], c["nodes"], **okw) for n, c in pick}
        _check_all(gpu_ctx, pick, want, results)
    _release(gpu_ctx, 2)


def _last_error(ctx):
    return ctx.lib.csm_last_error(ctx._ctx).decode()


def test_refusal_messages_are_the_single_call_s(cases):
    """A job refused in the middle of a batch leaves the message (and the status) the single call gives
    for it, whichever step refuses it: the node table (no nodes), the resize (flat box, no box, too
    large). With two refused jobs the message is the last one's in job order, as after the loop."""
    good = dict(cases)
    refused = _refused_cases() + [("no_nodes", dict(good["tiny"], nodes=[]))]
    a, b = api.Context(0), api.Context(0)
    try:
        single = {}
        for name, c in refused:
            with pytest.raises(api.CsmError) as err:
                a.construct_map_from_scans(BASE, c["shape"], c["map_pose"], c["nodes"])
            single[name] = (err.value.code, str(err.value).split(": ", 1)[1])
            assert single[name][1], name
        assert len({text for _, text in single.values()}) >= 3      # the messages tell the steps apart
        for name, c in refused:
            results, _ = b.construct_maps_from_scans(_jobs([("tiny", good["tiny"]), (name, c),
                                                            ("one_usable", good["one_usable"])]))
            assert [r[2] for r in results] == [0, single[name][0], 0], name
            assert _last_error(b) == single[name][1], name
        both = dict(refused)
        results, _ = b.construct_maps_from_scans(_jobs([("flat_box", both["flat_box"]), ("tiny", good["tiny"]),
                                                        ("too_large", both["too_large"])]))
        assert [r[2] for r in results] == [single["flat_box"][0], 0, single["too_large"][0]]
        assert _last_error(b) == single["too_large"][1] != single["flat_box"][1]
    finally:
        a.close()
        b.close()


def test_updates_onto_batch_built_maps(oracle, cases):
    """Context A builds three maps with the loop of single calls, context B with one batch call; then
    every map takes two csm_update_map_with_scan calls, one that fits and one that makes Expand grow
    the map (tests/map_batch_cases.py, update_nodes). After each step the two contexts hold the same
    shape, cells, first known row / column and counters, the cells are the oracle's, and at the end
    the cost / covariance, which reads the block allocation the updates carried, is bit-equal."""
    picked = [(n, c) for n, c in cases if n in MB.UPDATED]
    assert len(picked) == len(MB.UPDATED)
    keys = ("rays", "cell_updates", "saturated_reads", "first_known_row", "first_known_col", "device_projection")
    a, b = api.Context(0), api.Context(0)
    try:
        jobs = _jobs(picked)
        singles = [a.construct_map_from_scans(j["map_id"], j["shape"], j["map_pose"], j["nodes"]) for j in jobs]
        results, _ = b.construct_maps_from_scans(jobs)
        shapes, grids = [], []
        for j, (shape, _), (shape_b, _, status) in zip(jobs, singles, results):
            assert status == 0 and shape_b == shape
            shapes.append(shape)
            grids.append(a.download_level(j["map_id"], 0))
            assert np.array_equal(grids[-1], b.download_level(j["map_id"], 0))
        for step in range(2):
            for i, (j, (name, case)) in enumerate(zip(jobs, picked)):
                node = MB.update_nodes(case)[step]
                want_shape, want_grid, stats = oracle.update_map(shapes[i], grids[i], case["map_pose"], node)
                shape_a, info_a = a.update_map_with_scan(j["map_id"], shapes[i], case["map_pose"], node)
                shape_b, info_b = b.update_map_with_scan(j["map_id"], shapes[i], case["map_pose"], node)
                assert shape_a == shape_b == want_shape, (name, step)
                assert (shape_a != shapes[i]) == (step == 1), (name, step)
                for key in keys:
                    assert info_a[key] == info_b[key], (name, step, key)
                assert (info_a["rays"], info_a["cell_updates"], info_a["saturated_reads"]) == \
                    (stats["rays"], stats["updates"], stats["oob_reads"]), (name, step)
                got_a, got_b = a.download_level(j["map_id"], 0), b.download_level(j["map_id"], 0)
                assert np.array_equal(got_a, want_grid) and np.array_equal(got_b, want_grid), (name, step)
                assert a.debug_grid_known(j["map_id"]) == b.debug_grid_known(j["map_id"]), (name, step)
                shapes[i], grids[i] = want_shape, want_grid
        queries = _queries(picked, shapes)
        poses = [q["init_pose"] for q in queries]
        for ca, cb in zip(a.cost_covariance_batch(queries, poses, 1e4), b.cost_covariance_batch(queries, poses, 1e4)):
            assert np.isfinite(ca["normalized_cost"])
            assert np.array_equal(ca["normalized_cost"], cb["normalized_cost"], equal_nan=True)
            assert np.array_equal(ca["covariance"], cb["covariance"], equal_nan=True)
            assert np.array_equal(ca["hessian"], cb["hessian"], equal_nan=True)
    finally:
        a.close()
        b.close()
