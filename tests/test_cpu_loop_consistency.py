"""csm_host_loop_consistency against the independent literal (loop_consistency_reference.py): chi^2, adjacency
words, degrees, selected and info with ==, on every case and over the M ladder; the literal's Jacobians against
central differences; symmetry; the gates 0 and +inf; the seed counts; every refusal."""
import copy
import math

import numpy as np
import pytest

from csm_hip import api
import loop_consistency_reference as R


def _host(c, edges=None, gate=None, n_seeds=0, **kw):
    args = dict(R.drift_args(c))
    args.update(kw)
    return api.host_loop_consistency(c["local"], c["scan"], c["edges"] if edges is None else edges,
                                     c["gate"] if gate is None else gate, n_seeds=n_seeds, want_adjacency=True,
                                     want_chi2=True, **args)


def _same(got, want):
    """Every output of the library equals the literal's."""
    assert got["chi2"].shape == want["chi2"].shape
    assert got["chi2"].tobytes() == want["chi2"].tobytes()
    assert got["adjacency"].tobytes() == want["adjacency"].tobytes()
    assert got["degree"].tolist() == want["degree"].tolist()
    assert got["selected"].tolist() == want["selected"].tolist()
    assert got["info"] == want["info"]


@pytest.mark.parametrize("name", [n for n in R.CASES if n != "ladder"])
def test_host_function_is_the_literal(name):
    c = R.case(name)
    want = R.literal(c["local"], c["scan"], c["edges"], c["gate"], chi2=R.case_chi2(name))
    _same(_host(c), want)
    assert want["info"]["clique_size"] == int(want["selected"].sum()) >= 1


@pytest.mark.parametrize("m", R.LADDER)
def test_host_function_is_the_literal_over_the_ladder(m):
    c = R.case("ladder")
    n_seeds = 0 if m <= 65 else 3          # the literal's sets are slow: three searches at the large sizes
    want = R.literal(c["local"], c["scan"], c["edges"][:m], c["gate"], n_seeds=n_seeds,
                     chi2=R.prefix_chi2("ladder", m))
    got = _host(c, c["edges"][:m], n_seeds=n_seeds)
    _same(got, want)
    if m >= 63:                             # a ragged relation: neither empty nor one clique
        assert 0 < want["info"]["consistent_pairs"] < m * (m - 1) // 2
        assert 1 < want["info"]["clique_size"] < m


def test_separated_case_is_exactly_one_clique():
    """The condition for using the case: at gate 11.34 the inliers are pairwise consistent and no pair that
    touches an outlier is."""
    c = R.case("separated")
    chi, bad = R.case_chi2("separated")
    inl = ~c["outlier"]
    assert inl.sum() == 30 and bad == 0
    ok = chi <= c["gate"]
    np.fill_diagonal(ok, False)
    assert ok[np.ix_(inl, inl)].sum() == 30 * 29
    assert not ok[~inl, :].any() and not ok[:, ~inl].any()
    out = _host(c)
    assert out["selected"].tolist() == inl.astype(int).tolist()
    assert out["info"]["clique_size"] == 30 and out["info"]["consistent_pairs"] == 30 * 29 // 2
    assert out["degree"].tolist() == (29 * inl).tolist()


def test_peaks_of_one_pair_exclude_each_other():
    c = R.case("peaks")
    out = _host(c)
    p = c["peaks"]
    for a in p:
        for b in p:
            assert not (out["adjacency"][a, b >> 6] >> np.uint64(b & 63)) & np.uint64(1)
    assert out["selected"][p].sum() == 1 and out["selected"][p[0]] == 1
    assert out["info"]["clique_size"] == 12


def test_identical_edges_are_consistent_at_any_gate_above_rounding():
    """e of two identical edges is t_z - (R_B R_z R_z^T) t_z: zero but for the rounding of a rotation times its
    transpose, a few ulp of a metre; against a Sigma of 2.5e-3 m^2 that is a chi^2 below 1e-24."""
    c = R.case("duplicates")
    tiny = 1e-24
    out = _host(c, gate=tiny)
    pairs = {(i, j) for i in range(6) for j in range(i + 1, 6) if out["chi2"][i, j] <= tiny}
    assert pairs == set(c["same"])
    assert out["info"]["consistent_pairs"] == 4 and out["info"]["clique_size"] == 3
    assert out["selected"].tolist() == [1, 0, 1, 1, 0, 0]
    _same(_host(c, gate=0.0), R.literal(c["local"], c["scan"], c["edges"], 0.0, chi2=R.case_chi2("duplicates")))


def test_drift_model_makes_the_far_pair_consistent():
    c = R.case("drift")
    off = _host(c, drift_var_per_metre=None, local_travel=None, scan_travel=None)
    on = _host(c)
    _same(off, R.literal(c["local"], c["scan"], c["edges"], c["gate"]))
    _same(on, R.literal(c["local"], c["scan"], c["edges"], c["gate"], c["drift"], c["local_travel"], c["scan_travel"]))
    for i, j in c["flips"]:
        assert off["chi2"][i, j] > c["gate"] >= on["chi2"][i, j]
    assert off["chi2"][0, 2] <= c["gate"] and on["chi2"][0, 2] <= off["chi2"][0, 2]
    assert off["info"]["clique_size"] == 2 and on["info"]["clique_size"] == 3


def test_two_cliques_and_the_tie_rule():
    c = R.case("two_cliques")
    out = _host(c)
    assert out["info"]["clique_size"] == 7 and out["degree"].tolist() == [6] * 7 + [5] * 6
    assert out["selected"].tolist() == [1 if g == "a" else 0 for g in c["groups"]]
    c = R.case("two_cliques_equal")
    out = _host(c)
    assert out["degree"].tolist() == [5] * 12 and c["groups"][0] == "b"
    assert out["info"]["clique_size"] == 6 and out["info"]["winning_seed"] == 0
    assert out["selected"].tolist() == [1 if g == "b" else 0 for g in c["groups"]]


def test_bad_pivots_are_counted_and_inconsistent():
    c = R.case("bad_pivot")
    out = _host(c)
    m = len(c["edges"])
    assert out["info"]["bad_pivots"] == (m - 1) + (m - 2)
    for k in c["overflowing"]:
        assert out["degree"][k] == 0 and out["selected"][k] == 0
        assert np.isinf(np.delete(out["chi2"][k], k)).all() and out["chi2"][k, k] == 0.0
    inf = _host(c, gate=math.inf)           # +inf does not admit them either
    assert inf["info"]["consistent_pairs"] == (m - 2) * (m - 3) // 2 and inf["info"]["bad_pivots"] == 2 * m - 3


def test_an_indefinite_sum_is_a_bad_pivot_of_the_literal():
    """Built at the literal's level (no valid information matrix gives it): a Sigma with a negative eigenvalue."""
    c = R.case("separated")
    tab = [R.edge_table(c["local"], c["scan"], e, None, None) for e in c["edges"][:2]]
    assert R.pair_chi2(tab[0], tab[1], [0.0] * 3) is not None
    tab[0]["sigma"] = [[-1.0, 0.0, 0.0], [0.0, 1e-4, 0.0], [0.0, 0.0, 1e-4]]
    assert R.pair_chi2(tab[0], tab[1], [0.0] * 3) is None


def _perturbed(tab, which, k, h):
    t = copy.deepcopy(tab)
    t[which]["z"][k] += h
    t[which]["cz"], t[which]["sz"] = math.cos(t[which]["z"][2]), math.sin(t[which]["z"][2])
    return t


@pytest.mark.parametrize("pair", ((0, 1), (3, 8), (5, 30)))
def test_jacobians_of_the_literal_by_central_differences(pair):
    c = R.case("separated")
    tab = [R.edge_table(c["local"], c["scan"], c["edges"][k], None, None) for k in pair]
    _, Ji, Jj = R.cycle(tab[0], tab[1])
    h = 1e-6
    for which, J in ((0, Ji), (1, Jj)):
        for k in range(3):
            ep, _, _ = R.cycle(*_perturbed(tab, which, k, h))
            em, _, _ = R.cycle(*_perturbed(tab, which, k, -h))
            for r in range(3):
                d = ep[r] - em[r] if r < 2 else R.normalize_angle(ep[r] - em[r])
                # central differences of a smooth function of metres and radians at h = 1e-6: truncation
                # ~ h^2, rounding ~ 1e-16 * 10 m / h = 1e-9
                assert abs(d / (2.0 * h) - J[r][k]) < 1e-8


def test_outputs_are_symmetric():
    c = R.case("ladder")
    out = _host(c, c["edges"][:129], n_seeds=2)
    chi, adj = out["chi2"], out["adjacency"]
    assert chi.tobytes() == chi.T.copy().tobytes() and not chi.diagonal().any()
    bits = np.array([[(int(adj[i, j >> 6]) >> (j & 63)) & 1 for j in range(129)] for i in range(129)])
    assert (bits == bits.T).all() and not bits.diagonal().any()
    assert bits.sum(1).tolist() == out["degree"].tolist()
    assert not (int(adj[0, 2]) >> 1)                # no bit past M in the ragged last word
    sel = np.flatnonzero(out["selected"])
    assert bits[np.ix_(sel, sel)].sum() == sel.size * (sel.size - 1)      # a clique


def test_gate_zero_and_gate_infinity():
    c = R.case("ladder")
    e = c["edges"][:65]
    zero = _host(c, e, gate=0.0)
    assert zero["info"]["consistent_pairs"] == 0 and zero["info"]["clique_size"] == 1
    assert zero["selected"].tolist() == [1] + [0] * 64 and zero["info"]["winning_seed"] == 0
    inf = _host(c, e, gate=math.inf)
    assert inf["info"]["consistent_pairs"] == 65 * 64 // 2 and inf["selected"].all()
    _same(inf, R.literal(c["local"], c["scan"], e, math.inf, chi2=R.prefix_chi2("ladder", 65)))


def test_seed_counts():
    c = R.case("separated")
    m = len(c["edges"])
    chi = R.case_chi2("separated")
    for n in (1, 2, m, 0, m + 5):
        got = _host(c, n_seeds=n)
        _same(got, R.literal(c["local"], c["scan"], c["edges"], c["gate"], n_seeds=n, chi2=chi))
        assert got["info"]["seeds_run"] == (n if 0 < n < m else m)
    c = R.case("two_cliques_equal")         # one seed: only the first clique is ever searched
    assert _host(c, n_seeds=1)["info"]["winning_seed"] == 0


def test_one_edge_selects_itself():
    c = R.case("separated")
    out = _host(c, c["edges"][:1])
    assert out["selected"].tolist() == [1] and out["degree"].tolist() == [0]
    assert out["info"] == dict(consistent_pairs=0, bad_pivots=0, clique_size=1, winning_seed=0, seeds_run=1)
    assert out["chi2"].tolist() == [[0.0]] and out["adjacency"].tolist() == [[0]]


def _refused(c, edges=None, **kw):
    with pytest.raises(api.CsmError) as e:
        _host(c, edges, **kw)
    assert e.value.code == api.L.CSM_EINVAL


def test_every_refusal():
    c = R.case("drift")
    e = c["edges"]
    _refused(c, [])                                                          # M = 0
    _refused(c, [dict(e[0], local=12)] + e[1:])                              # an index out of range
    _refused(c, [dict(e[0], scan=-1)] + e[1:])
    _refused(c, [dict(e[0], scan=120)] + e[1:])
    _refused(c, [dict(e[0], rel=[0.0, math.nan, 0.0])] + e[1:])              # non-finite inputs
    _refused(c, [dict(e[0], info=np.diag([1.0, math.inf, 1.0]))] + e[1:])
    bad = c["scan"].copy()
    bad[7, 2] = math.inf
    with pytest.raises(api.CsmError):
        api.host_loop_consistency(c["local"], bad, e, c["gate"])
    bad = c["local"].copy()
    bad[3, 0] = math.nan
    with pytest.raises(api.CsmError):
        api.host_loop_consistency(bad, c["scan"], e, c["gate"])
    t = c["scan_travel"].copy()
    t[3] = math.nan
    _refused(c, scan_travel=t)
    _refused(c, gate=-1.0)                                                   # the gate
    _refused(c, gate=math.nan)
    _refused(c, drift_var_per_metre=[0.01, -0.01, 0.0])                      # the drift model
    _refused(c, drift_var_per_metre=[0.01, math.inf, 0.0])
    _refused(c, drift_var_per_metre=None)                                    # travel without variances
    _refused(c, local_travel=None)                                           # and the reverse
    _refused(c, scan_travel=None)
    _refused(c, n_seeds=-1)
    _refused(c, [dict(e[0], info=np.diag([1.0, -1.0, 1.0]))] + e[1:])        # a pivot of Lambda
    _refused(c, [dict(e[0], info=np.zeros((3, 3)))] + e[1:])
    many = [e[0]] * (api.L.LOOP_CONSISTENCY_MAX_EDGES + 1)                   # the caps
    with pytest.raises(api.CsmError):
        api.host_loop_consistency(c["local"], c["scan"], many, c["gate"])
    with pytest.raises(api.CsmError):
        api.host_loop_consistency(c["local"], c["scan"], many[:api.L.LOOP_CONSISTENCY_MAX_CHI2_EDGES + 1], c["gate"],
                                  want_chi2=True)
    assert _host(c)["info"]["clique_size"] == 3                              # and the call as it stands is fine


def test_edges_from_matches():
    c = R.case("separated")
    cov = np.diag(R.SIGMA ** 2)
    edges = api.loop_edges_from_matches([dict(local=e["local"], scan=e["scan"], pose=e["rel"], covariance=cov)
                                         for e in c["edges"]])
    a = api.host_loop_consistency(c["local"], c["scan"], edges, c["gate"], want_chi2=True)
    assert a["selected"].tolist() == (~c["outlier"]).astype(int).tolist()
    info = np.asarray(edges[0]["info"])
    assert info.tobytes() == info.T.copy().tobytes() and edges[0]["loop"]
