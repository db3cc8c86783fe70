"""csm_pose_graph_lm on the device, both solvers (the conjugate-gradient kernel k_pose_graph_lm and the
Schur-complement chain k_pgs_*), on the graph shapes of tests/pose_graph_cases.py, which
tests/test_cpu_pose_graph_cases.py pins to the Python literals on the host: nodes without edges,
repeated pairs, dense Schur complements, wrapped headings, b = 0, empty lists, edge / variable / block
counts at the kernels' strides, the launches after the step that stopped, and scratch kept between calls.

The comparisons are `_run_case` / `_compare` of test_gpu_pose_graph.py and test_gpu_pose_graph_schur.py
with their tolerances (POSE_ATOL, TOTAL_RTOL / TOTAL_ATOL, derived there): steps and lambda sequences
equal exactly, `_check_margins` on the host first.

One LM step is also held to a reference that shares no code with the library
(test_device_step_against_dense_solve): numpy.linalg.solve on pose_graph_literal.dense_system, squared
loss. Bound: ten times the host restatement's own error against that reference, measured on the CPU per
solver over the same four graphs (test_cpu_pose_graph_cases.py, DENSE_STEP_MEASURED):
  ConjugateGradient  measured 9.04143181090586e-14   bound 9.04e-13
  SchurCholesky      measured 2.4096331330503437e-14  bound 2.41e-13
relative to max|delta|. The host and the device differ in reduction order and 1-ulp sin / cos only,
which the spread studies of the two files above put near 1e-15 on one step. The device showed
(40 dense, 40 isolated, 330 dense, 330 isolated):
  ConjugateGradient  1.23e-14  1.28e-14  1.44e-14  1.00e-13
  SchurCholesky      1.27e-14  1.31e-14  1.59e-14  3.87e-14"""
import ctypes as C

import pytest

from csm_hip import _lib as L
from csm_hip import api, synth
import pose_graph_cases as PC
import test_gpu_pose_graph as CG
import test_gpu_pose_graph_schur as SC
from test_cpu_pose_graph import CASES, _case
from test_cpu_pose_graph_cases import DENSE_STEP_BOUND, DENSE_STEP_CASES, LAMBDA, dense_step, step_error

pytestmark = pytest.mark.gpu

SOLVERS = ("ConjugateGradient", "SchurCholesky")


def _run(ctx, c, solver, loss="Huber", **kw):
    """device against host with the solver's own comparison and tolerances"""
    return (CG if solver == "ConjugateGradient" else SC)._run_case(ctx, c, loss, **kw)


def _same_bits(a, b):
    return a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist() and a[2] == b[2]


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("n", [40, 330])
@pytest.mark.parametrize("name", PC.VARIANTS)
def test_variant_device_matches_host(gpu_ctx, name, n, solver):
    c = PC.case(n, name)
    (dl, ds, di), (hl, hs, hi) = _run(gpu_ctx, c, solver)
    if name == "isolated":
        for k in c["isolated_scans"]:
            assert ds[k].tolist() == c["scan"][k].tolist()
    elif name.startswith("idle_local"):
        assert dl[c["idle_local"]].tolist() == c["local"][c["idle_local"]].tolist()
    elif name == "zero":
        assert di["steps"] == 2 and all(t["rhs_norm2"] == 0.0 for t in di["trace"])
        assert dl.tolist() == c["local"].tolist() and ds.tolist() == c["scan"].tolist()
    elif name == "no_scan":
        assert (hi["steps"], hi["final_error"]) == (2, 0.0)
        for key in ("steps", "lambda_", "initial_error", "final_error"):
            assert di[key] == hi[key]
        assert dl.tolist() == c["local"].tolist() and ds.shape == (0, 3)


@pytest.mark.parametrize("solver", SOLVERS)
def test_dense_with_a_fourth_tile(gpu_ctx, solver):
    c = PC.case(490, "dense")
    assert len(c["local"]) == 49
    _run(gpu_ctx, c, solver)


# the strides of kPgsBlock = 256 (k_pgs_edges, k_pgs_error: nb_edges 1 -> 2 -> 3) and kPgBlock = 512
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("n_edges", [255, 256, 257, 512, 513])
def test_edge_count_at_block_boundaries(gpu_ctx, n_edges, solver):
    n = 200 if n_edges < 300 else 400
    c = PC.with_edge_count(synth.pose_graph_case(800 + n, n_scans=n, wrong_fraction=0.1), n_edges)
    assert PC.counts(c)[2] == n_edges
    _run(gpu_ctx, c, solver)


# 255, 256, 257 nodes: n_vars 765, 768, 771 and nb_vars (k_pgs_update's grid and partial sums) 3 -> 4
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("n_scans,n_vars", [(231, 765), (232, 768), (233, 771)])
def test_variable_count_at_block_boundaries(gpu_ctx, n_scans, n_vars, solver):
    c = synth.pose_graph_case(800 + n_scans, n_scans=n_scans, wrong_fraction=0.1)
    assert PC.counts(c)[1] == n_vars and (n_vars + 255) // 256 == (3 if n_vars <= 768 else 4)
    _run(gpu_ctx, c, solver)


# n_nodes + n_cross is the grid of k_pgs_assemble: one thread per diagonal or cross block
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("blocks", [767, 768, 769])
def test_block_count_at_grid_boundaries(gpu_ctx, blocks, solver):
    c = PC.with_block_count(PC.case(330), blocks)
    n_nodes, _, n_edges, n_cross = PC.counts(c)
    assert n_nodes + n_cross == blocks and n_cross == n_edges and 768 % 256 == 0
    _run(gpu_ctx, c, solver)


def test_schur_launches_after_the_stop_change_nothing(gpu_ctx):
    """Case 15 stops on ErrorTolerance = 1.0 before iterations_max = 10: the chain still launches the
    remaining steps' kernels, which must return at once. A call with iterations_max = steps launches
    none of them and must give the same bits."""
    seed, n, spm, wf, loss, scale, itmax, tol, lam, variant = CASES[14]
    assert (seed, itmax, tol) == (15, 10, 1.0)
    c = _case(seed, n, spm, wf, variant)
    dev, host = SC._run_case(gpu_ctx, c, loss, lam=lam, tol=tol, itmax=itmax)
    steps = dev[2]["steps"]
    assert 1 < steps < itmax and len(dev[2]["trace"]) == steps
    kw = dict(error_tolerance=tol, loss=loss, loss_scale=SC.LOSS_SCALE[loss], solver=SC.SOLVER)
    short = gpu_ctx.pose_graph_lm(c["local"], c["scan"], c["edges"], lam, iterations_max=steps, **kw)
    assert _same_bits(dev, short)
    # the trace array past `steps` is the caller's: the library leaves it alone
    ea = api.pose_graph_edges(c["edges"])
    lp, sp = c["local"].copy(), c["scan"].copy()
    trace = (L.PoseGraphLMStep * itmax)()
    for t in trace:
        t.total_error = -7.0
    lam_io, info = C.c_double(lam), L.PoseGraphLMInfo()
    params = api.pose_graph_params(iterations_max=itmax, **kw)
    rc = gpu_ctx.lib.csm_pose_graph_lm(gpu_ctx._ctx, api._ptr(lp), len(lp), api._ptr(sp), len(sp), ea, len(c["edges"]),
                                       C.byref(params), C.byref(lam_io), C.byref(info), trace)
    assert rc == 0 and info.steps == steps
    assert [t.total_error for t in trace[:steps]] == [t["total_error"] for t in dev[2]["trace"]]
    assert all(t.total_error == -7.0 for t in trace[steps:])


def test_schur_scratch_leaks_nothing_between_calls():
    """blocked (n_local 49), small (n_local 8), blocked again on one context: the first and the third
    result are equal bit for bit (S, wp, part and the state are rebuilt by every call), and the context
    gives back every byte when it is closed."""
    lib = L.load()
    d0, p0 = C.c_int64(), C.c_int64()
    assert lib.csm_debug_live_bytes(C.byref(d0), C.byref(p0)) == 0
    big, small = PC.case(490), PC.case(40)
    assert (len(big["local"]), len(small["local"])) == (49, 8)
    ctx = api.Context(0)
    try:
        a, _ = SC._run_case(ctx, big, "Huber")
        SC._run_case(ctx, small, "Huber")
        b = ctx.pose_graph_lm(big["local"], big["scan"], big["edges"], 1e-4, loss="Huber", loss_scale=0.01,
                              solver=SC.SOLVER)
        d1, p1 = C.c_int64(), C.c_int64()
        lib.csm_debug_live_bytes(C.byref(d1), C.byref(p1))
        assert d1.value - d0.value >= 8 * (3 * 49) ** 2
    finally:
        ctx.close()
    assert _same_bits(a, b)
    d2, p2 = C.c_int64(), C.c_int64()
    lib.csm_debug_live_bytes(C.byref(d2), C.byref(p2))
    assert (d2.value, p2.value) == (d0.value, p0.value)


# Case 19 (six scan nodes, no loop edge, tolerance 0) is a tree: its total error falls to ~1e-27 by the
# fourth step, far below TOTAL_ATOL, so from the third step on no seed keeps the decision margin. It
# runs with iterations_max 2 here; with tolerance 0 the stop rule still never fires.
CG_ITERATIONS_MAX = {19: 2}


@pytest.mark.parametrize("case", CASES, ids=[str(c[0]) for c in CASES])
def test_cpu_cases_on_the_conjugate_gradient_kernel(gpu_ctx, case):
    seed, n, spm, wf, loss, scale, itmax, tol, lam, variant = case
    c = _case(seed, n, spm, wf, variant)
    itmax = CG_ITERATIONS_MAX.get(seed, itmax)
    dev, host = CG._run_case(gpu_ctx, c, loss, lam=lam, tol=tol, itmax=itmax, scale=scale)
    assert dev[2]["steps"] == (itmax if tol == 0.0 else host[2]["steps"])
    if variant == "isolated":
        assert dev[1][n - 1].tolist() == c["scan"][n - 1].tolist()


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("n,name", DENSE_STEP_CASES)
def test_device_step_against_dense_solve(gpu_ctx, n, name, solver):
    """One squared-loss LM step of the device against numpy.linalg.solve on a dense H and b built by
    the Python literal: the only reference here that shares no arithmetic with the library. Bound
    (module docstring): ten times the host restatement's measured error, 9.04e-13 for the
    conjugate-gradient kernel and 2.41e-13 for the Schur chain, relative to max|delta|."""
    c = PC.case(n, name)
    want = dense_step(c)
    lp, sp, info = gpu_ctx.pose_graph_lm(c["local"], c["scan"], c["edges"], LAMBDA, iterations_max=1,
                                         loss="Squared", loss_scale=0.0, solver=solver)
    assert info["steps"] == 1
    err = step_error(c, lp, sp, want)
    print("relative error", err)
    assert err <= DENSE_STEP_BOUND[solver], err
    if name == "isolated":
        for k in c["isolated_scans"]:
            assert sp[k].tolist() == c["scan"][k].tolist()


@pytest.mark.parametrize("solver", SOLVERS)
def test_empty_edge_list_on_the_device(gpu_ctx, solver):
    """scan nodes but no edge (n_edges = 0 reaches the library behind api.pose_graph_edges' dummy
    element): the per-edge launches are skipped, every node is isolated, nothing moves"""
    c = PC.case(40)
    kw = dict(loss="Huber", loss_scale=0.01, solver=solver)
    hl, hs, hi = api.host_pose_graph_lm(c["local"], c["scan"], [], LAMBDA, **kw)
    dl, ds, di = gpu_ctx.pose_graph_lm(c["local"], c["scan"], [], LAMBDA, **kw)
    assert (hi["steps"], hi["initial_error"], hi["final_error"]) == (2, 0.0, 0.0)
    for key in ("steps", "lambda_", "initial_error", "final_error"):
        assert di[key] == hi[key]
    assert all(t["rhs_norm2"] == 0.0 and t["total_error"] == 0.0 for t in di["trace"])
    assert dl.tolist() == c["local"].tolist() and ds.tolist() == c["scan"].tolist()
