"""csm_host_pose_graph_marginals (the host restatement, the CPU reference of csm_pose_graph_marginals)
against the Python literal tests/pose_graph_marginals_literal.py bit for bit, the literal against
numpy.linalg.inv of the dense H (the two share no arithmetic), the refusals, and the host helpers that turn
a pair's relative covariance into a search window, a gate and a prior. CPU only.

The figures of LITERAL_ERROR (pose_graph_marginals_cases.py) are the literal's own largest error per case;
the host restatement is held to ten times the figure of its case."""
import copy
import math

import numpy as np
import pytest

from csm_hip import _lib as L
from csm_hip import api
import pose_graph_cases as PC
import pose_graph_marginals_cases as MC

IDS = ["%s-%s" % c for c in MC.CASES]


def _host(name, kind):
    c = MC.graph(name)
    return api.host_pose_graph_marginals(c["local"], c["scan"], c["edges"], MC.pairs(name, kind))


def _refused(c, pairs):
    with pytest.raises(api.CsmError) as ex:
        api.host_pose_graph_marginals(c["local"], c["scan"], c["edges"], pairs)
    assert ex.value.code == L.CSM_EINVAL


@pytest.mark.parametrize("case", MC.CASES, ids=IDS)
def test_host_marginals_match_the_literal_bit_for_bit(case):
    name, kind = case
    got, info = _host(name, kind)
    lit = MC.literal(name, kind)
    assert MC.same_bits(got, lit)
    assert all(r["finite"] == 1 for r in got)
    c, pairs = MC.graph(name), MC.pairs(name, kind)
    adj = MC.adjacency(c)
    cols = {s for s, _ in pairs} | {s for _, t in pairs if t is not None for s in adj[t]}
    assert info["n_columns"] == len(cols)
    for (s, t), r in zip(pairs, got):
        for k in ("local_cov", "scan_cov", "relative_cov"):
            assert np.array_equal(r[k], r[k].T)            # mirrored, so exactly symmetric
        if t is None:
            assert not r["scan_cov"].any() and not r["cross_cov"].any() and not r["relative_cov"].any()


@pytest.mark.parametrize("case", MC.CASES, ids=IDS)
def test_marginals_against_the_dense_inverse(case):
    name, kind = case
    lit = MC.error(MC.literal(name, kind), name, kind)
    host = MC.error(_host(name, kind)[0], name, kind)
    print("literal", lit, "recorded", MC.LITERAL_ERROR[case], "host", host)
    assert lit <= MC.bound(name, kind, 10.0)
    assert host <= MC.bound(name, kind, 10.0)


def test_single_edge_pair_has_the_edge_s_covariance():
    """One local map, one edge per scan node, no loop edge: x_t is tied to x_s by its edge alone, so the
    relative covariance of the pair is the inverse of the edge's information matrix; the anchor cancels."""
    c, pairs = MC.graph("star"), MC.pairs("star", "mixed")
    got, _ = _host("star", "mixed")
    worst, seen = 0.0, 0
    for (s, t), r in zip(pairs, got):
        if t is None:
            continue
        (edge,) = [e for e in c["edges"] if e["scan"] == t]
        want = np.linalg.inv(np.asarray(edge["info"], dtype=np.float64).reshape(3, 3))
        d = np.sqrt(np.diag(want))
        worst = max(worst, float((np.abs(r["relative_cov"] - want) / np.outer(d, d)).max()))
        seen += 1
    print("relative_cov against information^-1", worst)
    assert seen and worst <= MC.bound("star", "mixed", 10.0)


def test_a_pair_alone_among_all_and_reversed_has_the_same_bits():
    for name in ("plain17", "dense8"):
        c, pairs = MC.graph(name), MC.pairs(name, "mixed")
        whole, _ = api.host_pose_graph_marginals(c["local"], c["scan"], c["edges"], pairs)
        back, _ = api.host_pose_graph_marginals(c["local"], c["scan"], c["edges"], pairs[::-1])
        assert MC.same_bits(whole, back[::-1])
        for q, pair in enumerate(pairs):
            alone, info = api.host_pose_graph_marginals(c["local"], c["scan"], c["edges"], [pair])
            assert MC.same_bits(alone, whole[q:q + 1])


def test_graphs_without_a_gauge_path_are_refused():
    plain = MC.graph("synth2")
    _refused(PC.case(40, "idle_local_appended"), [(0, None)])
    _refused(PC.case(40, "idle_local_inserted"), [(0, None)])
    # the last local map cut off: its scan nodes keep only their edges to it
    c = copy.deepcopy(plain)
    last = len(c["local"]) - 1
    own = {e["scan"] for e in c["edges"] if e["local"] == last}
    c["edges"] = [e for e in c["edges"] if (e["scan"] not in own) or e["local"] == last]
    assert any(e["local"] == last for e in c["edges"])
    _refused(c, [(0, None)])
    api.host_pose_graph_marginals(plain["local"], plain["scan"], plain["edges"], [(0, None)])


def test_bad_pairs_are_refused():
    c = MC.graph("synth2")
    nl, nsn = len(c["local"]), len(c["scan"])
    for pairs in ([], [(-1, None)], [(nl, None)], [(0, -2)], [(0, nsn)], [(0, 0), (nl, 0)]):
        _refused(c, pairs)
    big = dict(local=np.zeros((L.PG_SCHUR_MAX_LOCAL + 1, 3)), scan=np.zeros((0, 3)), edges=[])
    _refused(big, [(0, None)])
    bad = copy.deepcopy(c)
    bad["scan"] = bad["scan"].copy()
    bad["scan"][3, 1] = math.inf
    _refused(bad, [(0, None)])
    with pytest.raises(api.CsmError):
        api.host_pose_graph_marginals(c["local"], c["scan"], c["edges"], [(0, None)], loss=9)


def test_scan_nodes_without_edges_named_and_unnamed():
    c = PC.case(40, "isolated")
    gone = c["isolated_scans"]
    _refused(c, [(0, gone[0])])
    _refused(c, [(1, 0), (0, gone[1])])
    # unnamed: the records are those of the graph without these scan nodes
    keep = [t for t in range(len(c["scan"])) if t not in gone]
    new = {t: q for q, t in enumerate(keep)}
    d = dict(local=c["local"], scan=c["scan"][keep], edges=[dict(e, scan=new[e["scan"]]) for e in c["edges"]])
    ts = [keep[0], keep[len(keep) // 2], keep[-1]]
    pairs = [(0, None)] + [(s, t) for t in ts for s in (0, 3, len(c["local"]) - 1)]
    with_idle, _ = api.host_pose_graph_marginals(c["local"], c["scan"], c["edges"], pairs)
    without, _ = api.host_pose_graph_marginals(d["local"], d["scan"], d["edges"], [(s, None if t is None else new[t])
                                                                                  for s, t in pairs])
    assert MC.same_bits(with_idle, without)


# ---------------------------------------------------------------- the helpers

def _relative_covs():
    got, _ = _host("synth3", "mixed")
    return [r["relative_cov"] for (s, t), r in zip(MC.pairs("synth3", "mixed"), got) if t is not None]


def test_loop_search_ranges_closed_form_and_clamps():
    lo, hi = [0.0, 0.0, 0.0], [1e9, 1e9, 1e9]
    for cov in _relative_covs():
        for n_sigma in (1.0, 3.0, 2.5):
            got = api.host_loop_search_ranges(cov, n_sigma, lo, hi)
            assert got.tolist() == [(2.0 * n_sigma) * math.sqrt(cov[a, a]) for a in range(3)]
    cov = np.diag([0.04, 1.0, 1e-6])
    got = api.host_loop_search_ranges(cov, 3.0, [0.5, 0.5, 0.05], [2.5, 2.5, 0.5])
    assert got.tolist() == [(2.0 * 3.0) * math.sqrt(0.04), 2.5, 0.05]
    assert api.host_loop_search_ranges(np.zeros((3, 3)), 3.0, lo, hi).tolist() == [0.0, 0.0, 0.0]
    for bad in (np.diag([1.0, -1e-12, 1.0]), np.diag([1.0, 1.0, math.nan]), np.diag([math.inf, 1.0, 1.0])):
        with pytest.raises(api.CsmError) as ex:
            api.host_loop_search_ranges(bad, 3.0, lo, hi)
        assert ex.value.code == L.CSM_EINVAL
    with pytest.raises(api.CsmError):
        api.host_loop_search_ranges(cov, math.nan, lo, hi)
    with pytest.raises(api.CsmError):
        api.host_loop_search_ranges(cov, 3.0, [1.0, 0.0, 0.0], [0.5, 1.0, 1.0])


def test_loop_gate_against_numpy():
    rng = np.random.RandomState(5)
    eps = 2.0 ** -52
    for cov in _relative_covs():
        m = rng.randn(3, 3) * 0.01
        match = m @ m.T + 1e-6 * np.eye(3)
        match = 0.5 * (match + match.T)
        pred = rng.randn(3)
        meas = pred + rng.randn(3) * 0.05
        got = api.host_loop_gate(cov, match, pred, meas)
        M = cov + match
        d = meas - pred
        want = float(d @ np.linalg.solve(M, d))
        # both solves are backward stable: a relative error of a few eps cond(M) each
        assert abs(got - want) <= 16.0 * eps * np.linalg.cond(M) * want, (got, want)
    # the heading difference is wrapped: 3.1 against -3.1 is 6.2 - 2 pi apart
    one = np.eye(3)
    got = api.host_loop_gate(one, np.zeros((3, 3)), [0.0, 0.0, -3.1], [0.0, 0.0, 3.1])
    assert got == (math.fmod(6.2, 2.0 * math.pi) - 2.0 * math.pi) ** 2
    assert api.host_loop_gate(one, one, [1.0, 2.0, 0.5], [1.0, 2.0, 0.5]) == 0.0
    for bad in (np.zeros((3, 3)), np.diag([1.0, -1.0, 1.0]), np.diag([1.0, 1.0, math.nan])):
        with pytest.raises(api.CsmError) as ex:
            api.host_loop_gate(bad, np.zeros((3, 3)), [0.0] * 3, [0.0] * 3)
        assert ex.value.code == L.CSM_EINVAL


def test_information_from_covariance_feeds_the_prior():
    eps = 2.0 ** -52
    for cov in _relative_covs():
        info = api.host_information_from_covariance(cov)
        assert np.array_equal(info, info.T)
        want = np.linalg.inv(cov)
        assert np.abs(info - want).max() <= 16.0 * eps * np.linalg.cond(cov) * np.abs(want).max()
        sensor = api.host_prior_from_robot_information(info, [0.4, -0.2, 0.3], [0.1, 0.05, 0.0])
        assert np.array_equal(np.asarray(sensor).reshape(3, 3), np.asarray(sensor).reshape(3, 3).T)
        q = api.host_motion_prior(sensor, (0.05, 0.05, 0.005), 360, 100)
        assert len(q) == 6
    for bad in (np.zeros((3, 3)), np.diag([1.0, 0.0, 1.0]), np.diag([1.0, 1.0, -2.0])):
        with pytest.raises(api.CsmError) as ex:
            api.host_information_from_covariance(bad)
        assert ex.value.code == L.CSM_EINVAL
