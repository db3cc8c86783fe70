"""Batches in which queries share one scan's arrays, the shape loop detection has and bench.py
times: the batch entries then stage the scan once (csm_batch.hip) and walk its finite check
once (same_scan, csm_plan.hip). The bench workload itself, built by bench.py's own functions on
a fresh context, is checked against the oracle and against the same batch with every query
holding its own copy of the arrays; smaller batches cover the other sharing patterns."""
import ctypes as C
import math

import numpy as np
import pytest

import bench
from csm_hip import api, synth

pytestmark = pytest.mark.gpu

CSM = (1.0, 1.0, math.radians(10), 4, 0.0, 0.0)


def _scan_ptrs(prepared):
    """(angles address, ranges address, n_points) of every query of a prepared batch."""
    return [(C.cast(q.scan.angles, C.c_void_p).value, C.cast(q.scan.ranges, C.c_void_p).value, q.scan.n_points)
            for q in prepared.arr]


def _copied(qs):
    return [dict(q, angles=np.copy(q["angles"]), ranges=np.copy(q["ranges"])) for q in qs]


def _case(ctx, q):
    return dict(grid=ctx.download_level(q["map_id"], 0), geom=q["geom"], angles=q["angles"], ranges=q["ranges"],
                rel_pose=q["rel_pose"], init_pose=q["init_pose"])


def _records(outs):
    return [(o["pose_found"], o["raw"], o["estimated_pose"]) for o in outs]


def _as_oracle(o, want):
    raw = o["raw"]
    assert o["pose_found"] == want["found"], (raw, want)
    assert (raw["best_x"], raw["best_y"], raw["best_theta"]) == (want["bestX"], want["bestY"], want["bestT"])
    assert raw["score"] == want["scoreMax"]
    assert o["estimated_pose"] == want["estimatedPose"]


def test_bench_loop_batch_equals_oracle_and_copied_scans(oracle):
    ctx = api.Context(0)
    try:
        qs, _ = bench.make_loop_queries(ctx, 0, 256)
        prepared = ctx.prepare_queries(qs)
        ptrs = _scan_ptrs(prepared)
        assert len(set(ptrs)) == 1, "the bench queries no longer share one scan's arrays"
        outs = ctx.bnb_match_batch(prepared, *bench.LOOP_PARAMS, as_records=True)
        got = _records(outs)
        for i in range(0, 256, 8):
            c = synth.make_room(100000 + i, half_x=bench.LOOP_ROOM[0], half_y=bench.LOOP_ROOM[1])
            case = _case(ctx, qs[i])
            assert np.array_equal(case["grid"], c[0])
            _as_oracle(outs[i], oracle.bnb(case, *bench.LOOP_PARAMS))
        copied = ctx.prepare_queries(_copied(qs))
        assert len(set(_scan_ptrs(copied))) == 256
        assert _records(ctx.bnb_match_batch(copied, *bench.LOOP_PARAMS, as_records=True)) == got
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def small():
    """Eight resident maps of the loop family and two scans of their room."""
    ctx = api.Context(0)
    maps = []
    for i in range(8):
        grid, geom, _ = synth.make_room(100000 + i, half_x=bench.LOOP_ROOM[0], half_y=bench.LOOP_ROOM[1])
        ctx.upload_grid(i, grid)
        maps.append((grid, geom))
    scans = [bench.loop_scan(0), bench.loop_scan(1)]
    yield ctx, maps, scans
    ctx.close()


def _query(maps, i, scan, k, angles=None, ranges=None, rel_pose=(0.0, 0.0, 0.0)):
    truth, a, r = scan
    rng = np.random.RandomState(5000 + 17 * i + k)
    init = tuple(np.asarray(truth) + rng.uniform(-0.3, 0.3, 3) * (1, 1, 0.15))
    return dict(map_id=i, geom=maps[i][1], angles=a if angles is None else angles,
                ranges=r if ranges is None else ranges, rel_pose=rel_pose, init_pose=init)


def _both_matchers(ctx, oracle, qs):
    """bnb_match_batch and correlative_match_batch on the batch as given and on copied arrays:
    equal records, each equal to the oracle."""
    out = {}
    for name, run, lit, prm in (("bnb", ctx.bnb_match_batch, oracle.bnb, bench.LOOP_PARAMS),
                                ("csm", ctx.correlative_match_batch, oracle.csm, CSM)):
        shared = run(ctx.prepare_queries(qs), *prm)
        assert _records(run(ctx.prepare_queries(_copied(qs)), *prm)) == _records(shared), name
        for q, o in zip(qs, shared):
            _as_oracle(o, lit(_case(ctx, q), *prm))
        out[name] = shared
    return out


def test_non_adjacent_repeats_of_a_scan(small, oracle):
    """A A B A B: one device copy per scan, but the finite check only skips adjacent repeats."""
    ctx, maps, (sa, sb) = small
    order = [sa, sa, sb, sa, sb, sa, sb, sb]
    qs = [_query(maps, i, s, 0) for i, s in enumerate(order)]
    prepared = ctx.prepare_queries(qs)
    assert len(set(_scan_ptrs(prepared))) == 2
    _both_matchers(ctx, oracle, qs)


def test_one_scan_with_a_relative_pose_per_query(small, oracle):
    ctx, maps, (sa, _) = small
    qs = [_query(maps, i, sa, 1, rel_pose=(0.02 * i, -0.01 * i, 0.01 * (i % 3))) for i in range(8)]
    _both_matchers(ctx, oracle, qs)


def test_one_scan_with_a_prefix_per_query(small, oracle):
    """The same arrays, different n_points (prefix views: same data pointer)."""
    ctx, maps, (sa, _) = small
    _, a, r = sa
    qs = [_query(maps, i, sa, 2, angles=a[:len(a) - 97 * (i % 4)], ranges=r[:len(r) - 97 * (i % 4)])
          for i in range(8)]
    ptrs = _scan_ptrs(ctx.prepare_queries(qs))
    assert len({p[:2] for p in ptrs}) == 1 and len({p[2] for p in ptrs}) == 4
    _both_matchers(ctx, oracle, qs)


@pytest.mark.parametrize("bad", [0, 3, 7])
def test_shared_scan_with_a_nan_names_the_same_query(small, bad):
    """A NaN in a scan shared by some queries of an otherwise valid batch: the error names the
    same (first) query index as with every query holding its own copy."""
    ctx, maps, (sa, sb) = small
    truth, a, r = sa
    r_bad = np.copy(r)
    r_bad[11] = np.nan
    bad_scan = (truth, a, r_bad)
    qs = [_query(maps, i, bad_scan if i >= bad and i % 2 == bad % 2 else sb, 3) for i in range(8)]
    for run, prm in ((ctx.bnb_match_batch, bench.LOOP_PARAMS), (ctx.correlative_match_batch, CSM)):
        msgs = []
        for batch in (qs, _copied(qs)):
            with pytest.raises(api.CsmError) as e:
                run(batch, *prm)
            msgs.append(str(e.value))
        assert "query %d:" % bad in msgs[0], msgs
        assert msgs[0] == msgs[1]


def test_repeated_batch_then_one_submap_updated(small, oracle):
    """The same prepared batch twice, then again after update_map_with_scan on one submap: only
    that query's record may change, and it equals the oracle on the updated map."""
    ctx, maps, (sa, _) = small
    mc = synth.map_case(940, n_scans=3, n_beams=360, max_range=5.0)
    shape, _ = ctx.construct_map_from_scans(8, mc["shape"], mc["map_pose"], mc["nodes"][:2])
    qs = [_query(maps, i, sa, 4) for i in range(8)]
    nd, mp = mc["nodes"][2], mc["map_pose"]
    c, s = math.cos(mp[2]), math.sin(mp[2])
    dx, dy = nd["pose"][0] + 0.05 - mp[0], nd["pose"][1] - 0.04 - mp[1]
    init8 = (c * dx + s * dy, -s * dx + c * dy, nd["pose"][2] + 0.02 - mp[2])     # map-local
    geom8 = (shape["res"], shape["off_x"], shape["off_y"])
    qs.append(dict(map_id=8, geom=geom8, angles=nd["angles"], ranges=nd["ranges"], rel_pose=nd["rel_pose"],
                   init_pose=init8))
    matchers = (("bnb", ctx.bnb_match_batch, oracle.bnb, bench.LOOP_PARAMS),
                ("csm", ctx.correlative_match_batch, oracle.csm, CSM))
    prepared = ctx.prepare_queries(qs)
    first = {}
    for name, run, lit, prm in matchers:
        first[name] = _records(run(prepared, *prm))
        outs = run(prepared, *prm)
        assert _records(outs) == first[name]
        for q, o in zip(qs, outs):
            _as_oracle(o, lit(_case(ctx, q), *prm))
    # one more scan on submap 8, same frame: the map changes in place under the same id
    grid_before = ctx.download_level(8, 0)
    shape2, grid2, _ = oracle.update_map(shape, grid_before, mc["map_pose"], mc["nodes"][1])
    got_shape, _ = ctx.update_map_with_scan(8, shape, mc["map_pose"], mc["nodes"][1])
    assert got_shape == shape2 == shape
    assert np.array_equal(ctx.download_level(8, 0), grid2)
    assert not np.array_equal(grid2, grid_before)
    for name, run, lit, prm in matchers:
        after = run(prepared, *prm)
        assert _records(after)[:8] == first[name][:8]
        _as_oracle(after[8], lit(_case(ctx, qs[8]), *prm))
    ctx.release_grid(8)
