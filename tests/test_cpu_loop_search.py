"""csm_host_loop_search, csm_host_travel_distances and csm_host_loop_candidates_nearest against the literal
statement of the rule (loop_search_reference.py), byte for byte, and the nearest form against a literal walk
of LoopSearcherNearest::Search. No GPU."""
import numpy as np
import pytest

from csm_hip import _lib as L
from csm_hip import api
import loop_search_cases as LC
import loop_search_reference as R

KS = (1, 2, 16)


def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype.itemsize == b.dtype.itemsize and a.shape == b.shape and a.tobytes() == b.tobytes()


def _host(c, q, qt, k, one_per_map, n_ref=None, **kw):
    args = dict(travel_dist_threshold=c["travel_dist_threshold"], node_dist_threshold=c["node_dist_threshold"],
                n_per_query=k, one_per_map=one_per_map)
    args.update(kw)
    return api.host_loop_search(c["poses"], c["map_index"], c["travel"], q, qt, n_ref, **args)


def test_layouts_and_limits_are_the_header_s():
    assert R.CANDIDATE.itemsize == 24 and api.LOOP_CANDIDATE_DTYPE == R.CANDIDATE
    assert (L.LOOP_SEARCH_MAX_K, R.MAX_K) == (16, 16)


def test_the_laps_family_holds_what_it_must():
    shows = LC.laps_properties(16)
    assert all(v is not None for v in shows.values())
    assert LC.laps_properties(1)["tie_at_cut"] is not None


@pytest.mark.parametrize("name", LC.FAMILIES)
def test_travel_distances_are_the_literal_accumulation(name):
    c = LC.family(name)
    got = api.host_travel_distances(c["poses"])
    assert _same_bytes(got, c["travel"])
    assert np.all(np.diff(got) >= 0)
    assert api.host_travel_distances(np.zeros((0, 3))).size == 0
    assert api.host_travel_distances([[1.0, 2.0, 3.0]]).tolist() == [0.0]


def test_far_frame_travel_is_the_laps_travel():
    assert _same_bytes(LC.family("far_frame")["travel"], LC.family("laps")["travel"])


@pytest.mark.parametrize("one_per_map", (False, True))
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", LC.FAMILIES)
def test_host_search_is_the_rule_byte_for_byte(name, k, one_per_map):
    c = LC.family(name)
    q, qt = LC.all_queries(c)
    rec, counts, info = _host(c, q, qt, k, one_per_map)
    want, wcounts, winfo = R.rule(c["poses"], c["map_index"], c["travel"], len(q), q, qt, c["travel_dist_threshold"],
                                  c["node_dist_threshold"], k, one_per_map)
    assert _same_bytes(rec, want)
    assert _same_bytes(counts, wcounts)
    assert info == winfo
    assert info["pairs_eligible"] > 0 and info["pairs_evaluated"] > info["pairs_eligible"]


def test_far_frame_records_are_the_laps_records():
    a, b = LC.family("laps"), LC.family("far_frame")
    q, qt = LC.all_queries(a)
    ra, ca, ia = _host(a, q, qt, 16, False)
    rb, cb, ib = _host(b, q, qt, 16, False)
    assert _same_bytes(ra, rb) and _same_bytes(ca, cb) and ia == ib


@pytest.mark.parametrize("name", LC.FAMILIES)
def test_shuffled_queries_and_a_reference_limit(name):
    c = LC.family(name)
    n = len(c["poses"])
    rng = np.random.default_rng(5)
    q = rng.permutation(n).astype(np.int32)[: n // 2]
    qt = c["travel"][q] + rng.uniform(-3.0, 3.0, q.size)
    n_ref = (2 * n) // 3
    rec, counts, info = _host(c, q, qt, 2, False, n_ref=n_ref)
    want, wcounts, winfo = R.rule(c["poses"], c["map_index"], c["travel"], n_ref, q, qt, c["travel_dist_threshold"],
                                  c["node_dist_threshold"], 2, False)
    assert _same_bytes(rec, want) and _same_bytes(counts, wcounts) and info == winfo
    assert rec["ref_scan_index"].max() < n_ref


def _online(c, last):
    lo, hi = c["runs"][last]
    q = np.arange(lo, hi + 1, dtype=np.int32)
    return q, float(c["travel"][hi]), lo


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", LC.FAMILIES)
def test_nearest_form_is_the_reference_s_candidate_set(name, k):
    c = LC.family(name)
    checked = 0
    for last in (len(c["runs"]) - 1, len(c["runs"]) // 2, (3 * len(c["runs"])) // 4):
        q, accum, n_ref = _online(c, last)
        rec, counts, _ = _host(c, q, np.full(q.size, accum), k, False, n_ref=n_ref)
        got = api.host_loop_candidates_nearest(rec, counts, k)
        assert _same_bytes(got, R.nearest(rec, counts, k))
        walk = R.reference_walk(c["poses"], c["runs"], accum, last, c["travel_dist_threshold"],
                                c["node_dist_threshold"])
        tie = len(walk) > k and walk[k - 1][0] == walk[k][0]
        if name == "random_walk":
            assert not tie              # compared as the reference would return it
        # with a tie at the cut nth_element may keep any of the equal pairs: the walk's fully sorted prefix
        # is the one this library specifies; without one it is the reference's own set
        want = {(qq, rr, mm) for _, rr, qq, mm in walk[:k]}
        assert {(int(g["query_scan_index"]), int(g["ref_scan_index"]), int(g["ref_map_index"])) for g in got} == want
        assert [float(g["dist_sq"]) for g in got] == [w[0] for w in walk[:k]]
        checked += len(walk) > 0
    assert checked > 0


def test_nearest_takes_fewer_than_asked_and_none():
    c = LC.family("laps")
    q, qt = LC.all_queries(c)
    rec, counts, _ = _host(c, q[:200], qt[:200], 2, False)
    total = int(counts.sum())
    assert 0 < total < 400 and (counts == 0).any()
    assert api.host_loop_candidates_nearest(rec, counts, 400).size == total
    assert api.host_loop_candidates_nearest(rec, counts, 0).size == 0
    with pytest.raises(api.CsmError):
        api.host_loop_candidates_nearest(rec, counts + 3, 4)
    with pytest.raises(api.CsmError):
        api.host_loop_candidates_nearest(rec, counts, -1)


@pytest.mark.parametrize("name", LC.FAMILIES)
def test_one_per_map_keeps_the_first_of_each_map(name):
    c = LC.family(name)
    q, qt = LC.all_queries(c)
    full, fcounts, _ = _host(c, q, qt, 16, False)
    uncut = 0
    for k in KS:
        rec, counts, _ = _host(c, q, qt, k, True)
        for i in range(len(q)):
            maps = rec[i, :counts[i]]["ref_map_index"].tolist()
            assert len(set(maps)) == len(maps)
            if fcounts[i] < 16:         # the full list is not cut: the per-map records are a subsequence of it
                uncut += 1
                firsts, seen = [], set()
                for cand in full[i, :fcounts[i]]:
                    if int(cand["ref_map_index"]) not in seen:
                        seen.add(int(cand["ref_map_index"]))
                        firsts.append(cand)
                assert _same_bytes(rec[i, :counts[i]], np.array(firsts[:k], R.CANDIDATE).reshape(-1))
    assert uncut > 0


def _refused(c, **change):
    q, qt = LC.all_queries(c)
    a = dict(poses=c["poses"].copy(), map_index=c["map_index"].copy(), travel=c["travel"].copy(), q=q[-20:].copy(),
             qt=qt[-20:].copy(), n_ref=None, n_maps=None, travel_dist_threshold=10.0, node_dist_threshold=2.0,
             n_per_query=2, one_per_map=False)
    for key, v in change.items():
        if callable(v):
            v(a[key])
        else:
            a[key] = v
    try:
        api.host_loop_search(a["poses"], a["map_index"], a["travel"], a["q"], a["qt"], a["n_ref"],
                             a["travel_dist_threshold"], a["node_dist_threshold"], a["n_per_query"],
                             a["one_per_map"], a["n_maps"])
    except api.CsmError as e:
        return e.code == L.CSM_EINVAL
    return False


def _put(index, value):
    def change(a):
        a[index] = value
    return change


REFUSALS = {
    "accepted as it is": None,
    "a pose x that is NaN": dict(poses=_put((5, 0), np.nan)),
    "a pose y that is infinite": dict(poses=_put((7, 1), np.inf)),
    "a travel value that is NaN": dict(travel=_put(3, np.nan)),
    "a travel value that is infinite": dict(travel=_put(-1, np.inf)),
    "a query travel that is NaN": dict(qt=_put(0, np.nan)),
    "a travel threshold that is infinite": dict(travel_dist_threshold=np.inf),
    "a node threshold that is NaN": dict(node_dist_threshold=np.nan),
    "travel decreasing": dict(travel=_put(100, 0.0)),
    "map index decreasing": dict(map_index=_put(100, 3)),
    "a map index below zero": dict(map_index=_put(0, -1)),
    "a map index at n_maps": dict(n_maps=38),
    "n_maps zero": dict(n_maps=0),
    "n_maps above the limit": dict(n_maps=L.LOOP_SEARCH_MAX_MAPS + 1),
    "n_ref below zero": dict(n_ref=-1),
    "n_ref above n_scan": dict(n_ref=385),
    "a query index below zero": dict(q=_put(2, -1)),
    "a query index at n_scan": dict(q=_put(2, 384)),
    "a query index repeated": dict(q=_put(2, 383)),
    "no query": dict(q=np.zeros(0, np.int32), qt=np.zeros(0)),
    "n_per_query zero": dict(n_per_query=0),
    "n_per_query above the limit": dict(n_per_query=17),
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusals(what):
    c = LC.family("laps")
    assert len(c["poses"]) == 384 and c["map_index"][-1] == 38
    if REFUSALS[what] is None:
        assert not _refused(c)
    else:
        assert _refused(c, **REFUSALS[what])


def test_the_node_limit_is_refused():
    n = L.LOOP_SEARCH_MAX_NODES + 1
    with pytest.raises(api.CsmError):
        api.host_loop_search(np.zeros((n, 3)), np.zeros(n, np.int32), np.zeros(n), [0], [0.0])


def test_graph_arrays_of_a_search_hint():
    c = LC.family("laps")
    sp, mi, tr, n_ref, q = api.loop_search_graph(c["poses"], c["runs"], 20)
    assert len(sp) == 210 and n_ref == 200 and q.tolist() == list(range(200, 210))
    assert _same_bytes(mi, c["map_index"][:210]) and _same_bytes(tr, c["travel"][:210])
    for bad in ([(0, 9), (11, 20)], [(1, 9)], [(0, 9), (10, 400)]):
        with pytest.raises(api.CsmError):
            api.loop_search_graph(c["poses"], bad, len(bad) - 1)
    with pytest.raises(api.CsmError):
        api.loop_search_graph(c["poses"], c["runs"], len(c["runs"]))
