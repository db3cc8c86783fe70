"""The premises of tests/test_gpu_mixed_batch.py, checked without a GPU: the pool of
tests/mixed_batch_cases.py really forms several groups per call (loop_batch's key: the padded
leaf-window extents), neighbours in the input order usually fall in different groups, and the
group-wide decisions of csm_batch.hip's BatchGroup::plan meet queries they were not taken from:
fine.weighted from the first query (merging_pays), two_rounds from any query's min_known, the
bound pass's limit on n_theta_max."""
import math

import numpy as np

from csm_hip import api

import mixed_batch_cases as mb

RX = RY = 1.0
RT = math.radians(10)


def _key(unit):
    return lambda q: mb.group_key(q, api.host_search_step, api.host_window, RX, RY, unit)


def _units():
    # correlative batch: unit L; branch and bound: unit 2^H
    return [L for L in (1, 3, 4, 5)] + [1 << H for H in (0, 2, 4)]


def test_pool_is_deterministic():
    a, b = mb.make_pool(0), mb.make_pool(0)
    assert [q["name"] for q in a["queries"]] == [q["name"] for q in b["queries"]]
    for qa, qb in zip(a["queries"], b["queries"]):
        assert np.array_equal(qa["angles"], qb["angles"]) and np.array_equal(qa["ranges"], qb["ranges"])
        assert qa["init_pose"] == qb["init_pose"] and qa["map_id"] == qb["map_id"]
    for mid in a["maps"]:
        assert np.array_equal(a["maps"][mid]["grid"], b["maps"][mid]["grid"])


def test_pool_holds_every_kind_of_map_and_scan():
    pool = mb.make_pool(0)
    qs, maps = pool["queries"], pool["maps"]
    assert {m["geom"][0] for m in maps.values()} == set(mb.RES)
    shapes = [m["grid"].shape for m in maps.values()]
    assert any(r % 64 or c % 64 for r, c in shapes)
    assert any(max(r, c) >= 5 * min(r, c) for r, c in shapes)           # long and thin
    assert sum(m["blocks"] is not None for m in maps.values()) == 1
    blocks = next(m["blocks"] for m in maps.values() if m["blocks"] is not None)
    assert any(b is None for b in blocks[0]) and any(b is not None for b in blocks[0])
    beams = {len(q["angles"]) for q in qs}
    assert {1, 7, 360, 1080, 5000} <= beams
    assert any(max(q["ranges"]) == 20.0 for q in qs) and any(max(q["ranges"]) < 6.0 for q in qs)
    assert any(any(v != 0.0 for v in q["rel_pose"]) for q in qs)
    per_map = {}
    for q in qs:
        per_map[q["map_id"]] = per_map.get(q["map_id"], 0) + 1
    assert max(per_map.values()) >= 3
    # one query is off its map: every beam of every candidate reads outside it
    off = [q for q in qs if q["name"] == "b_off"][0]
    g = maps[off["map_id"]]
    res, ox, oy = g["geom"]
    rows, cols = g["grid"].shape
    x, y = off["init_pose"][:2]
    reach = max(off["ranges"]) + RX          # the longest beam from the farthest candidate
    assert x - reach > ox + cols * res or y + reach < oy
    # scans shared within a group and across groups are the same numpy objects
    by_id = {}
    for i, q in enumerate(qs):
        by_id.setdefault(id(q["angles"]), []).append(i)
    shared = [ix for ix in by_id.values() if len(ix) > 1]
    assert shared
    key = _key(4)
    assert any(len({key(qs[i]) for i in ix}) > 1 for ix in shared)          # across groups
    assert any(len({key(qs[i]) for i in ix}) < len(ix) for ix in shared)    # within a group


def test_every_call_forms_several_groups_in_interleaved_order():
    qs = mb.make_pool(0)["queries"]
    for unit in _units():
        key = _key(unit)
        groups = mb.groups_in_order(qs, key)
        assert len(groups) >= 3, unit
        keys = [key(q) for q in qs]
        differ = sum(keys[i] != keys[i + 1] for i in range(len(keys) - 1))
        assert 2 * differ >= len(keys) - 1, (unit, keys)


def test_two_rounds_meets_queries_that_do_not_need_it():
    """With a known-rate threshold, one group holds a query whose min_known is at most one (its
    coarse pass only runs on the edge band) and one whose min_known is above one (two_rounds)."""
    qs = mb.make_pool(0)["queries"]
    key = _key(4)
    for thr in (0.3, 0.6):
        mixed = 0
        for ix in mb.groups_in_order(qs, key).values():
            mk = [api.host_min_known(len(qs[i]["angles"]), thr) for i in ix]
            mixed += min(mk) <= 1 < max(mk)
        assert mixed >= 2, thr


def test_first_query_decides_weighting_for_a_mixed_group():
    """In one group merging_pays holds for the first query and not for the last: the forward batch
    runs the group with weighted lists (joint kernels, bound pass), the reversed one without."""
    qs = mb.make_pool(0)["queries"]
    pays = [mb.merging_pays(q["angles"], q["ranges"], q["geom"][0]) for q in qs]
    for unit in _units():
        groups = mb.groups_in_order(qs, _key(unit)).values()
        assert any(pays[ix[0]] and not pays[ix[-1]] for ix in groups), unit
        assert sum(any(pays[i] for i in ix) and not all(pays[i] for i in ix) for ix in groups) >= 2


def test_long_range_call_crosses_the_bound_pass_limit():
    """range_theta = 2 pi: the 20 m scan's group needs more than 2048 slices (bound pass off:
    (n_theta_max + 1) / 2 > 1024) while its neighbours need about 700."""
    pool = mb.make_pool(0)
    sub = mb.long_range_subset(pool)
    nt = {q["name"]: mb.n_theta(q, api.host_search_step, api.host_window, 2 * math.pi) for q in sub}
    assert max(nt.values()) > 2048
    assert any(600 <= v <= 800 for v in nt.values())
    key = _key(4)
    groups = mb.groups_in_order(sub, key)
    assert len(groups) >= 3
    long_group = next(ix for ix in groups.values() if any(sub[i]["name"] == "b_long" for i in ix))
    assert min(nt[sub[i]["name"]] for i in long_group) < 1024
    assert "b_5000" not in nt
