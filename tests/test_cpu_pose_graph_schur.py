"""The host restatement of PoseGraphOptimizerLM::Optimize with the direct Schur-complement Cholesky
solver (csm_host_pose_graph_lm, CSM_PG_SOLVER_SCHUR_CHOLESKY) against the Python literal
(tests/pose_graph_schur_literal.py) bit for bit, against numpy on one step, and against the
conjugate-gradient solver. CPU only: it is the reference the GPU tests hold the device to."""
import copy

import numpy as np
import pytest

from csm_hip import _lib as L
from csm_hip import api
import pose_graph_literal as PL
import pose_graph_schur_literal as SL
from test_cpu_pose_graph import CASES, _assert_same, _case
from test_gpu_pose_graph import _check_margins

IDS = [str(c[0]) for c in CASES]

# Item "residual": the largest residual_norm2 / rhs_norm2 that the Python literal (not the library)
# shows over the twenty CASES is 9.063279157428158e-27 (case 18); the library may show ten times that.
LITERAL_RESIDUAL_RATIO = 9.063279157428158e-27
RESIDUAL_RATIO_BOUND = 10.0 * LITERAL_RESIDUAL_RATIO

# Direct against conjugate gradient: with the two Python literals (pose_graph_literal.optimize and
# pose_graph_schur_literal.optimize) on synth.pose_graph_case graphs of 20, 60, 150 and 400 scan nodes
# (seed 300 + n), all six losses at 20 - 150 (Huber, Squared and Welsch at 400), wrong loop fraction
# 0 and 0.2, every run took the same steps with the same lambdas and the largest
# max |pose_direct - pose_cg| was 7.105427357601002e-15 (150 scan nodes, Welsch). Bound: 100x.
DIRECT_VS_CG_MEASURED = 7.105427357601002e-15
DIRECT_VS_CG_ATOL = 100.0 * DIRECT_VS_CG_MEASURED


def _host(c, lam, loss, scale, itmax, tol, solver="SchurCholesky"):
    return api.host_pose_graph_lm(c["local"], c["scan"], c["edges"], lam, iterations_max=itmax,
                                  error_tolerance=tol, loss=loss, loss_scale=scale, solver=solver)


def _literal(c, lam, loss, scale, itmax, tol):
    return SL.optimize(c["local"].tolist(), c["scan"].tolist(), c["edges"], lam, itmax, tol, loss, scale)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_schur_matches_literal_bit_for_bit(case):
    seed, n, spm, wf, loss, scale, itmax, tol, lam, variant = case
    c = _case(seed, n, spm, wf, variant)
    got = _host(c, lam, loss, scale, itmax, tol)
    lit = _literal(c, lam, loss, scale, itmax, tol)
    _assert_same(got, lit)
    info = got[2]
    assert info["cg_iterations"] == 0 and all(t["cg_iterations"] == 0 for t in info["trace"])
    if variant == "zero":
        assert all(t["rhs_norm2"] == 0.0 and t["residual_norm2"] == 0.0 for t in info["trace"])
        assert got[0].tolist() == c["local"].tolist()
        assert got[1].tolist() == c["scan"].tolist()
    if itmax == 3:
        assert info["steps"] == 3
    if tol == 1.0:
        tr = info["trace"]
        assert info["steps"] < itmax and abs(tr[-1]["total_error"] - tr[-2]["total_error"]) < tol
    if variant == "isolated":
        assert got[1][n - 1].tolist() == c["scan"][n - 1].tolist()


def test_schur_lambda_carries_over_two_calls():
    c = _case(21, 24, 6, 0.2, None)
    lp, sp, i1 = _host(c, 1e-4, "Huber", 0.01, 10, 1e-4)
    lp2, sp2, i2 = api.host_pose_graph_lm(lp, sp, c["edges"], i1["lambda_"], solver="SchurCholesky")
    assert i2["trace"][0]["lambda_"] == i1["lambda_"]
    a = _literal(c, 1e-4, "Huber", 0.01, 10, 1e-4)
    b = SL.optimize(a[0], a[1], c["edges"], a[2], 10, 1e-4, "Huber", 0.01)
    _assert_same((lp2, sp2, i2), b)


def test_schur_step_solves_the_normal_equations():
    """One LM step against numpy.linalg.solve on a dense copy of H and b, with the bound the
    conjugate-gradient test uses (1e-9 max|delta| + 1e-14)."""
    c = _case(23, 30, 6, 0.1, None)
    lam = 1e-3
    H, b = PL.dense_system(c["local"].tolist(), c["scan"].tolist(), c["edges"], lam)
    want = np.linalg.solve(H, b)
    lp, sp, info = _host(c, lam, "Huber", 0.01, 1, 1e-4)
    got = np.concatenate([(lp - c["local"]).ravel(), (sp - c["scan"]).ravel()])
    scale = np.abs(want).max()
    assert np.abs(got - want).max() <= 1e-9 * scale + 1e-14, (np.abs(got - want).max(), scale)
    t = info["trace"][0]
    assert t["rhs_norm2"] == float(sum(v * v for v in b.tolist()))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_schur_residual_is_small(case):
    """residual_norm2 = |b - H delta|^2 is the solver's self-check: at most ten times the largest
    ratio to rhs_norm2 that the Python literal shows over these cases (9.063279157428158e-27)."""
    seed, n, spm, wf, loss, scale, itmax, tol, lam, variant = case
    c = _case(seed, n, spm, wf, variant)
    lit = _literal(c, lam, loss, scale, itmax, tol)
    ratio = max((t[3] / t[2] if t[2] else 0.0) for t in lit[3])
    print("literal ratio", ratio)
    assert ratio <= LITERAL_RESIDUAL_RATIO
    for t in _host(c, lam, loss, scale, itmax, tol)[2]["trace"]:
        print("library ratio", t["residual_norm2"] / t["rhs_norm2"] if t["rhs_norm2"] else 0.0)
        assert t["residual_norm2"] <= RESIDUAL_RATIO_BOUND * t["rhs_norm2"]


def _has_margin(info, tol):
    try:
        _check_margins(info, tol)
    except AssertionError:
        return False
    return True


def test_schur_agrees_with_conjugate_gradient():
    """Both solvers on the host, the twenty CASES: where every LM decision of both runs has the margin
    the device test demands, the steps and the lambda sequence are equal; the poses of runs that took
    the same decisions agree within DIRECT_VS_CG_ATOL = 100 x 7.105427357601002e-15, the largest
    difference between the two Python literals (see the constants above). At most a quarter of the
    cases may lack the margin."""
    without_margin = []
    for case in CASES:
        seed, n, spm, wf, loss, scale, itmax, tol, lam, variant = case
        c = _case(seed, n, spm, wf, variant)
        d = _host(c, lam, loss, scale, itmax, tol)
        g = _host(c, lam, loss, scale, itmax, tol, solver="ConjugateGradient")
        lam_d = [t["lambda_"] for t in d[2]["trace"]]
        lam_g = [t["lambda_"] for t in g[2]["trace"]]
        if _has_margin(d[2], tol) and _has_margin(g[2], tol):
            assert d[2]["steps"] == g[2]["steps"], seed
            assert lam_d == lam_g and d[2]["lambda_"] == g[2]["lambda_"], seed
        else:
            without_margin.append(seed)
        if lam_d == lam_g:
            diff = max(np.abs(d[0] - g[0]).max(), np.abs(d[1] - g[1]).max())
            print("case", seed, "max |direct - cg|", diff)
            assert diff <= DIRECT_VS_CG_ATOL, (seed, diff)
    assert len(without_margin) <= len(CASES) // 4, without_margin


def _expect_einval(c, lam=1e-4, **kw):
    with pytest.raises(api.CsmError) as ex:
        api.host_pose_graph_lm(c["local"], c["scan"], c["edges"], lam, solver="SchurCholesky", **kw)
    assert ex.value.code == L.CSM_EINVAL


def test_schur_einval_paths():
    c = _case(22, 12, 4, 0.0, None)
    # more local map nodes than the dense Schur complement allows, one scan node
    big = dict(local=np.zeros((L.PG_SCHUR_MAX_LOCAL + 1, 3)), scan=np.zeros((1, 3)),
               edges=[dict(local=0, scan=0, rel=[0.0, 0.0, 0.0], info=np.eye(3), loop=False)])
    _expect_einval(big)
    lp, sp, info = api.host_pose_graph_lm(big["local"][:8], big["scan"], big["edges"], 1e-4, solver="SchurCholesky")
    assert info["steps"] >= 1
    _expect_einval(c, iterations_max=0)
    _expect_einval(c, loss=9)
    _expect_einval(c, loss="Cauchy", loss_scale=-1.0)
    _expect_einval(c, lam=float("nan"))
    for field, val in (("local", 3), ("local", -1), ("scan", 12)):
        d = copy.deepcopy(c)
        d["edges"][2][field] = val
        _expect_einval(d)
    d = copy.deepcopy(c)
    d["scan"][5, 2] = float("inf")
    _expect_einval(d)
    d = copy.deepcopy(c)
    d["local"][1, 0] = float("nan")
    _expect_einval(d)
    d = copy.deepcopy(c)
    d["edges"][3]["rel"][1] = float("nan")
    _expect_einval(d)
    d = copy.deepcopy(c)
    d["edges"][3]["info"] = np.array(d["edges"][3]["info"])
    d["edges"][3]["info"][1, 1] = float("inf")
    _expect_einval(d)
    d = copy.deepcopy(c)
    d["local"] = d["local"][:0]
    d["edges"] = []
    _expect_einval(d)
    with pytest.raises(api.CsmError):
        api.host_pose_graph_lm(c["local"], c["scan"], c["edges"], 1e-4, solver=3)
    with pytest.raises(api.CsmError):
        api.host_pose_graph_lm(c["local"], c["scan"], c["edges"], 1e-4, solver="SparseCholesky")
