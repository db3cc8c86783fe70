"""The graph shapes of tests/pose_graph_cases.py on the CPU: every variant reaches the shape it is
named for, the host restatement csm_host_pose_graph_lm equals both Python literals
(pose_graph_literal.py, pose_graph_schur_literal.py) on it bit for bit, every LM decision of the host
has the margin the device tests demand, and one LM step of the host solves the normal equations that
numpy.linalg.solve solves (the source of the device test's bound)."""
import math

import numpy as np
import pytest

from csm_hip import api
import pose_graph_cases as PC
import pose_graph_literal as PL
import pose_graph_schur_literal as SL
import test_gpu_pose_graph as CG
import test_gpu_pose_graph_schur as SC
from test_cpu_pose_graph import _assert_same

SOLVERS = {"ConjugateGradient": (PL, CG), "SchurCholesky": (SL, SC)}
LOSS, SCALE, LAMBDA, TOL, ITMAX = "Huber", 0.01, 1e-4, 1e-4, 10

# One LM step against numpy.linalg.solve (see test_host_step_against_dense_solve): the largest
# max|delta_host - delta_dense| / max|delta_dense| of the host restatement per solver over the four
# graphs, and ten times that as the bound for the host here and for the device.
DENSE_STEP_CASES = [(40, "dense"), (40, "isolated"), (330, "dense"), (330, "isolated")]
DENSE_STEP_MEASURED = {"ConjugateGradient": 9.04143181090586e-14, "SchurCholesky": 2.4096331330503437e-14}
DENSE_STEP_BOUND = {k: 10.0 * v for k, v in DENSE_STEP_MEASURED.items()}


def _host(c, solver, itmax=ITMAX, loss=LOSS, scale=SCALE):
    return api.host_pose_graph_lm(c["local"], c["scan"], c["edges"], LAMBDA, iterations_max=itmax,
                                  error_tolerance=TOL, loss=loss, loss_scale=scale, solver=solver)


@pytest.mark.parametrize("solver", list(SOLVERS))
@pytest.mark.parametrize("name", PC.VARIANTS)
def test_host_matches_literal_bit_for_bit_on_variant(name, solver):
    c = PC.case(40, name)
    lit = SOLVERS[solver][0].optimize(c["local"].tolist(), c["scan"].tolist(), c["edges"], LAMBDA, ITMAX, TOL,
                                      LOSS, SCALE)
    got = _host(c, solver)
    _assert_same(got, lit)
    if name in ("zero", "no_scan"):
        assert got[2]["steps"] == 2 and got[2]["final_error"] == 0.0
        assert all(t["rhs_norm2"] == 0.0 and t["cg_iterations"] == 0 for t in got[2]["trace"])
        assert got[0].tolist() == c["local"].tolist() and got[1].tolist() == c["scan"].tolist()


@pytest.mark.parametrize("n", [40, 330])
@pytest.mark.parametrize("name", PC.VARIANTS)
def test_variant_reaches_its_shape(name, n):
    base, c = PC.case(n), PC.case(n, name)
    nl, ns = len(base["local"]), len(base["scan"])
    dl, ds = PC.degrees(c)
    pairs = PC.pair_counts(c)
    # the plain graph is the chain the variants leave: one to three edges per scan node, no idle node,
    # no repeated pair, headings that grow past pi
    bl, bs = PC.degrees(base)
    assert min(bl) >= 1 and 1 <= min(bs) and max(bs) <= 3
    assert max(PC.pair_counts(base).values()) == 1
    assert base["scan"][:, 2].max() > math.pi
    assert nl == {40: 8, 330: 33}[n] and (3 * nl <= SC.SMALL) == (n == 40)
    if name == "isolated":
        mid, last = c["isolated_scans"]
        assert 0 < mid < last == ns - 1 and ds[mid] == ds[last] == 0
        assert sum(1 for d in ds if d == 0) == 2 and min(dl) >= 1
    elif name.startswith("idle_local"):
        at = c["idle_local"]
        assert len(c["local"]) == nl + 1 and dl[at] == 0
        assert at == (nl if name.endswith("appended") else nl // 2)
        assert [d for k, d in enumerate(dl) if k != at] == bl and ds == bs
        assert max(e["local"] for e in c["edges"]) == (nl - 1 if name.endswith("appended") else nl)
    elif name == "dense":
        lists = PC.schur_list_lengths(c)
        assert len(lists) == nl * (nl + 1) // 2             # every block of S is stored
        assert max(lists.values()) >= ns / 4 and min(ds) >= nl // 2
        assert len(c["edges"]) >= len(base["edges"]) + ns * (nl // 2)
    elif name == "dup":
        assert len(c["edges"]) == len(base["edges"]) + (len(base["edges"]) + 2) // 3
        assert max(pairs.values()) == 2 and sum(1 for v in pairs.values() if v == 2) >= len(base["edges"]) // 3
    elif name == "wrapped":
        th = np.concatenate([c["local"][:, 2], c["scan"][:, 2]])
        assert th.max() <= math.pi and th.min() > -math.pi
        assert np.abs(np.sin(th) - np.sin(np.concatenate([base["local"][:, 2], base["scan"][:, 2]]))).max() < 1e-14
        cross = [e for e in c["edges"]
                 if abs(c["scan"][e["scan"], 2] - c["local"][e["local"], 2] - e["rel"][2]) > math.pi]
        assert len(cross) >= 3                              # d2 - z2 leaves (-pi, pi] on these edges
    elif name == "zero":
        assert len(c["edges"]) == len(base["edges"]) and not c["local"][:, 2].any()
    elif name == "one_local":
        assert len(c["local"]) == 1 and dl == [len(base["edges"])] and max(pairs.values()) >= 2
    elif name == "no_scan":
        assert len(c["local"]) == nl and c["scan"].shape == (0, 3) and c["edges"] == []
    # the precondition of the device tests, on the sizes they run
    for solver, (_, mod) in SOLVERS.items():
        mod._check_margins(_host(c, solver)[2], TOL)


def test_dense_with_a_fourth_tile():
    c = PC.case(490, "dense")
    nl = len(c["local"])
    assert nl == 49 and math.ceil(3 * nl / SC.TILE) == 4
    lists = PC.schur_list_lengths(c)
    assert len(lists) == nl * (nl + 1) // 2 and max(lists.values()) >= 490 / 4
    for solver, (_, mod) in SOLVERS.items():
        mod._check_margins(_host(c, solver)[2], TOL)


def test_edge_and_block_count_helpers():
    c = PC.case(330)
    n_nodes, n_vars, n_edges, n_cross = PC.counts(c)
    assert (n_nodes, n_vars) == (363, 1089) and n_cross == n_edges
    for want in (n_edges - 7, n_edges, n_edges + 9):
        d = PC.with_edge_count(c, want)
        assert PC.counts(d)[2] == want
        assert PC.counts(d)[3] == min(want, n_edges)        # a duplicate adds no cross block
        kept = min(want, n_edges)
        assert [(e["local"], e["scan"], e["rel"]) for e in d["edges"] if not e["loop"]] == \
            [(e["local"], e["scan"], e["rel"]) for e in c["edges"] if not e["loop"]]
        assert all(e["loop"] for e in d["edges"][kept:])
    d = PC.with_block_count(c, 768)
    assert PC.counts(d)[0] + PC.counts(d)[3] == 768
    assert len(c["edges"]) == n_edges                       # the shared graph is left alone


@pytest.mark.parametrize("solver", list(SOLVERS))
@pytest.mark.parametrize("n,name", DENSE_STEP_CASES)
def test_host_step_against_dense_solve(n, name, solver):
    """One LM step with the squared loss (no edge weight enters): delta = new poses - old poses against
    numpy.linalg.solve on pose_graph_literal.dense_system. H carries 1e9 on node 0 and lambda = 1e-4 on
    an isolated node, so its condition number (4e6 dense, 1e13 isolated) decides the bound, not a round
    figure. Measured max|delta_host - delta_dense| / max|delta_dense| of the host restatement:
                         40 dense   40 isolated   330 dense   330 isolated
      ConjugateGradient  1.23e-14   1.55e-14      1.47e-14    9.04e-14
      SchurCholesky      1.27e-14   1.31e-14      1.80e-14    2.41e-14
    The bound is ten times the largest per solver (DENSE_STEP_BOUND: 9.04e-13 and 2.41e-13), far below
    the 1e-9 that test_converged_step_solves_the_normal_equations allows on a plain graph. The device
    test (test_gpu_pose_graph_cases.py) holds the device to the same bound."""
    c = PC.case(n, name)
    want = dense_step(c)
    lp, sp, info = _host(c, solver, itmax=1, loss="Squared", scale=0.0)
    assert info["steps"] == 1
    err = step_error(c, lp, sp, want)
    print("relative error", err)
    assert err <= DENSE_STEP_BOUND[solver], err
    assert DENSE_STEP_BOUND[solver] < 1e-9


_dense = {}


def dense_step(c):
    """numpy.linalg.solve(H, b) of one squared-loss step at the graph's initial poses; once per graph"""
    if id(c) not in _dense:
        H, b = PL.dense_system(c["local"].tolist(), c["scan"].tolist(), c["edges"], LAMBDA, loss_kind="Squared",
                               loss_scale=0.0)
        assert np.array_equal(H, H.T)
        _dense[id(c)] = np.linalg.solve(H, b)
    return _dense[id(c)]


def step_error(c, lp, sp, want):
    got = np.concatenate([(lp - c["local"]).ravel(), (sp - c["scan"]).ravel()])
    return float(np.abs(got - want).max() / np.abs(want).max())


@pytest.mark.parametrize("solver", list(SOLVERS))
def test_empty_edge_list_reaches_the_library(solver):
    """api.pose_graph_edges allocates one dummy element for an empty list; the library must still be
    told n_edges = 0. With n_scan = 0 a dummy edge (scan node 0) would be refused as out of range."""
    assert len(api.pose_graph_edges([])) == 1
    c = PC.case(40, "no_scan")
    lp, sp, info = _host(c, solver)
    assert (info["steps"], info["initial_error"], info["final_error"]) == (2, 0.0, 0.0)
    assert info["lambda_"] == LAMBDA * 0.5 and sp.shape == (0, 3) and lp.tolist() == c["local"].tolist()
    # scan nodes, but no edge: every node is isolated
    base = PC.case(40)
    lp, sp, info = api.host_pose_graph_lm(base["local"], base["scan"], [], LAMBDA, solver=solver)
    assert (info["steps"], info["initial_error"], info["final_error"]) == (2, 0.0, 0.0)
    assert lp.tolist() == base["local"].tolist() and sp.tolist() == base["scan"].tolist()
