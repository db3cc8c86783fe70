"""Single-query launch chains replayed as HIP graphs (csm_correlative_match, from the third query
of a launch shape on): the records must equal those of the kernel-by-kernel path and the oracle,
for varying scans and poses of one shape, for alternating shapes, across a map re-upload, and for
integer-key ties resolved right after a replay (single queries and repeated batches)."""
import math

import numpy as np
import pytest

from csm_hip import _lib as L, api, synth

pytestmark = pytest.mark.gpu


def _match(ctx, case, sc, rx, ry, rt, Lr):
    return ctx.correlative_match(1, case["geom"], sc["angles"], sc["ranges"], case["rel_pose"], sc["init_pose"],
                                 rx, ry, rt, Lr, 0.0, 0.0)


def test_graph_replay_equals_plain_launches(oracle):
    case = synth.csm_case(31, n_beams=720)
    rng = np.random.RandomState(5)
    scans = []
    for k in range(10):
        truth = (0.3 * (rng.rand() - 0.5), 0.3 * (rng.rand() - 0.5), 0.2 * (rng.rand() - 0.5))
        angles, ranges = synth.cast_scan(case["segs"], truth, 720, 2 * math.pi, 5.7296)
        init = (truth[0] + 0.1, truth[1] - 0.08, truth[2] + 0.02)
        scans.append(dict(angles=angles, ranges=ranges, init_pose=init))
    graphs = api.Context(0)
    plain = api.Context(0, tuning_off=L.TUNE_NO_GRAPHS)
    for c in (graphs, plain):
        c.upload_grid(1, case["grid"])
    shapes = [(1.0, 1.0, math.radians(10), 4), (0.6, 0.8, math.radians(6), 4)]
    for rep in range(3):                       # every shape is seen often enough to be recorded and replayed
        for sc in scans:
            for rx, ry, rt, Lr in shapes:
                a = _match(graphs, case, sc, rx, ry, rt, Lr)
                b = _match(plain, case, sc, rx, ry, rt, Lr)
                assert a["raw"] == b["raw"] and a["estimated_pose"] == b["estimated_pose"]
                if rep == 2:
                    c2 = dict(case, angles=sc["angles"], ranges=sc["ranges"], init_pose=sc["init_pose"])
                    lit = oracle.csm(c2, rx, ry, rt, Lr)
                    assert (a["raw"]["best_x"], a["raw"]["best_y"], a["raw"]["best_theta"], a["raw"]["score"]) == \
                        (lit["bestX"], lit["bestY"], lit["bestT"], lit["scoreMax"])
    # a new map under the same id (the frontend re-uploads its latest map before every match)
    case2 = synth.csm_case(32, n_beams=720)
    for c in (graphs, plain):
        c.upload_grid(1, case2["grid"])
    for sc in scans[:4]:
        a = _match(graphs, case2, sc, *shapes[0])
        b = _match(plain, case2, sc, *shapes[0])
        assert a["raw"] == b["raw"]
    graphs.close()
    plain.close()


def _tie_cases():
    """Two maps of the same size whose best integer key is shared by several candidates
    (quantised to two levels, no unknown interior), with different contents."""
    return synth.csm_case(42, levels=2, interior_unknown=0.0), synth.csm_case(40, levels=2, interior_unknown=0.0)


def _match_on(ctx, map_id, case, rx, ry, rt, Lr):
    return ctx.correlative_match(map_id, case["geom"], case["angles"], case["ranges"], case["rel_pose"],
                                 case["init_pose"], rx, ry, rt, Lr, 0.0, 0.0)


def _same_record(a, b):
    assert a["raw"] == b["raw"], (a["raw"], b["raw"])
    assert a["estimated_pose"] == b["estimated_pose"]


def _as_oracle(out, lit):
    raw = out["raw"]
    assert out["pose_found"] == lit["found"], (raw, lit)
    assert (raw["best_x"], raw["best_y"], raw["best_theta"]) == (lit["bestX"], lit["bestY"], lit["bestT"]), (raw, lit)
    assert raw["score"] == lit["scoreMax"]
    assert out["estimated_pose"] == lit["estimatedPose"]


def test_graph_replay_resolves_ties_on_its_own_map(oracle):
    """A A A B A A B A on two same-size resident maps, one window shape: from the third query of a
    map on its chain is a replayed graph, and the tie collection pass after a replay must score the
    replayed map, not the map of the last kernel-by-kernel launch."""
    ca, cb = _tie_cases()
    assert ca["grid"].shape == cb["grid"].shape
    prm = (1.0, 1.0, math.radians(10), 4)
    want = {1: oracle.csm(ca, *prm), 2: oracle.csm(cb, *prm)}
    cases = {1: ca, 2: cb}
    graphs = api.Context(0)
    plain = api.Context(0, tuning_off=L.TUNE_NO_GRAPHS)
    for c in (graphs, plain):
        c.upload_grid(1, ca["grid"])
        c.upload_grid(2, cb["grid"])
    # one query of each map first: every workspace (the tie pass's included) has its size, so the
    # graph keys, which carry the allocation epoch, stay the same from here on
    for map_id in (2, 1):
        _match_on(graphs, map_id, cases[map_id], *prm)
    seq = (1, 1, 1, 2, 1, 1, 2, 1)
    replayed = []
    for map_id in seq:
        case = cases[map_id]
        a = _match_on(graphs, map_id, case, *prm)
        info = graphs.last_search_info()
        b = _match_on(plain, map_id, case, *prm)
        assert plain.last_search_info()["graph_replayed"] == 0
        assert info["two_phase"] == 0
        replayed.append(info["graph_replayed"])
        _same_record(a, b)
        _as_oracle(a, want[map_id])
        assert a["raw"]["tie_count"] > 1, a["raw"]
    # map 1 is recorded by its third query at the latest; the queries right after map 2's are replays
    assert replayed[4] == 1 and replayed[7] == 1, replayed
    assert replayed[3] == 0, replayed
    graphs.close()
    plain.close()


def test_batch_tie_queries_repeated_on_one_context(oracle):
    """The batch entries finish every KEY_TIE record with the single-query path, so a batch that
    is repeated on one context replays graphs once their keys are stable. Six calls of one batch
    (tie queries on same-size maps, ordinary queries between them): every record equals the
    oracle's and the first call's."""
    ctx = api.Context(0)
    ca, cb = _tie_cases()
    cases = [ca, synth.csm_case(33, n_beams=360), cb, synth.csm_case(131, levels=2, interior_unknown=0.0),
             synth.csm_case(34, n_beams=540)]
    qs = []
    for i, c in enumerate(cases):
        ctx.upload_grid(20 + i, c["grid"])
        qs.append(dict(map_id=20 + i, geom=c["geom"], angles=c["angles"], ranges=c["ranges"],
                       rel_pose=c["rel_pose"], init_pose=c["init_pose"]))
    prm = (1.0, 1.0, math.radians(10), 4, 0.0, 0.0)
    want = [oracle.csm(c, *prm) for c in cases]
    prepared = ctx.prepare_queries(qs)
    first = None
    for call in range(6):
        outs = ctx.correlative_match_batch(prepared, *prm)
        for o, w in zip(outs, want):
            _as_oracle(o, w)
        ties = sum(o["raw"]["flags"] & L.FLAG_KEY_TIE != 0 for o in outs)
        assert ties >= 2, [o["raw"] for o in outs]
        if first is None:
            first = outs
        for o, f in zip(outs, first):
            _same_record(o, f)
    # the last tie query of the last call was a replay (its key's fourth call or later)
    assert ctx.last_search_info()["graph_replayed"] == 1
    ctx.close()
