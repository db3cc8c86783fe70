"""The library's host restatement of PoseGraphOptimizerLM::Optimize (csm_host_pose_graph_lm)
against the Python literal (tests/pose_graph_literal.py), bit for bit: poses, every trace field,
the initial error and the final lambda. CPU only: it is the reference the GPU tests hold the
device to."""
import copy
import math

import numpy as np
import pytest

from csm_hip import _lib as L
from csm_hip import api, synth
import pose_graph_literal as PL
from pose_graph_cases import zero_rhs as _zero_rhs


def _dup_edges(c):
    """the first odometry edge and one loop edge (if any) appended again: H sums duplicates"""
    c = copy.deepcopy(c)
    extra = [copy.deepcopy(c["edges"][1])]
    loops = [e for e in c["edges"] if e["loop"]]
    if loops:
        extra.append(copy.deepcopy(loops[0]))
    c["edges"] += extra
    return c


# (seed, scans, scans per map, wrong loop fraction, loss, scale, iterations max, error tolerance, lambda, variant)
CASES = [
    (1, 4, 10, 0.0, "Huber", 0.01, 10, 1e-4, 1e-4, None),
    (2, 12, 4, 0.0, "Squared", 0.0, 10, 1e-4, 1e-4, None),
    (3, 24, 5, 0.2, "Huber", 0.01, 10, 1e-4, 1e-4, None),
    (4, 24, 5, 0.2, "Cauchy", 0.05, 10, 1e-4, 1e-4, None),
    (5, 24, 5, 0.2, "Fair", 0.1, 10, 1e-4, 1e-4, None),
    (6, 24, 5, 0.2, "GemanMcClure", 0.5, 10, 1e-4, 1e-4, None),
    (7, 24, 5, 0.2, "Welsch", 1.0, 10, 1e-4, 1e-4, None),
    (8, 30, 6, 0.0, "Squared", 0.0, 10, 1e-4, 1e-3, None),
    (9, 30, 6, 0.3, "Huber", 1.0, 10, 1e-4, 1e-4, None),
    (10, 20, 5, 0.0, "Huber", 0.01, 10, 1e-4, 1e-4, "dup"),
    (11, 20, 5, 0.2, "Cauchy", 0.01, 10, 1e-4, 1e-4, "dup"),
    (12, 9, 50, 0.0, "Huber", 0.01, 10, 1e-4, 1e-4, None),         # one local map
    (13, 18, 4, 0.0, "Huber", 0.01, 10, 1e-4, 1e-4, "zero"),       # b = 0: CG early return
    (14, 30, 5, 0.1, "Huber", 0.01, 3, 1e-4, 1e-4, None),          # stops on NumOfIterationsMax
    (15, 30, 5, 0.1, "Huber", 0.01, 10, 1.0, 1e-4, None),          # stops on ErrorTolerance early
    (16, 40, 8, 0.1, "Welsch", 0.2, 10, 1e-4, 10.0, None),         # heavy damping
    (17, 16, 4, 0.0, "Fair", 0.01, 1, 1e-4, 1e-4, None),           # a single step
    (18, 36, 6, 0.25, "GemanMcClure", 0.05, 10, 1e-6, 1e-5, None),
    (19, 6, 3, 0.0, "Squared", 0.0, 10, 0.0, 1e-4, None),          # tolerance 0: runs every step
    (20, 33, 7, 0.15, "Huber", 0.01, 10, 1e-4, 1e-4, "isolated"),  # a scan node without edges
]


def _case(seed, n, spm, wf, variant):
    c = synth.pose_graph_case(seed, n_scans=n, scans_per_map=spm, lap_scans=max(6, n // 2), wrong_fraction=wf)
    if variant == "dup":
        c = _dup_edges(c)
    elif variant == "zero":
        c = _zero_rhs(c)
    elif variant == "isolated":
        gone = n - 1
        c["edges"] = [e for e in c["edges"] if e["scan"] != gone]
    return c


def _host(c, lam, loss, scale, itmax, tol):
    return api.host_pose_graph_lm(c["local"], c["scan"], c["edges"], lam, iterations_max=itmax,
                                  error_tolerance=tol, loss=loss, loss_scale=scale)


def _literal(c, lam, loss, scale, itmax, tol):
    return PL.optimize(c["local"].tolist(), c["scan"].tolist(), c["edges"], lam, itmax, tol, loss, scale)


def _assert_same(got, lit):
    lp, sp, info = got
    llp, lsp, llam, ltrace, linit = lit
    assert lp.tolist() == llp
    assert sp.tolist() == lsp
    assert info["lambda_"] == llam
    assert info["initial_error"] == linit
    assert [(t["total_error"], t["lambda_"], t["rhs_norm2"], t["residual_norm2"], t["cg_iterations"])
            for t in info["trace"]] == ltrace
    assert info["steps"] == len(ltrace)
    assert info["final_error"] == ltrace[-1][0]
    assert info["cg_iterations"] == sum(t[4] for t in ltrace)


@pytest.mark.parametrize("case", CASES, ids=[str(c[0]) for c in CASES])
def test_host_restatement_matches_literal_bit_for_bit(case):
    seed, n, spm, wf, loss, scale, itmax, tol, lam, variant = case
    c = _case(seed, n, spm, wf, variant)
    got = _host(c, lam, loss, scale, itmax, tol)
    lit = _literal(c, lam, loss, scale, itmax, tol)
    _assert_same(got, lit)
    info = got[2]
    if wf > 0:
        assert any(e["loop"] for e in c["edges"])
    if variant == "zero":
        assert all(t["cg_iterations"] == 0 and t["rhs_norm2"] == 0.0 for t in info["trace"])
        assert got[1].tolist() == c["scan"].tolist()
    if itmax == 3:
        assert info["steps"] == 3          # NumOfIterationsMax
    if tol == 1.0:
        tr = info["trace"]
        assert info["steps"] < itmax and abs(tr[-1]["total_error"] - tr[-2]["total_error"]) < tol
    if variant == "isolated":
        assert got[1][n - 1].tolist() == c["scan"][n - 1].tolist()


def test_lambda_carries_over_two_calls():
    c = _case(21, 24, 6, 0.2, None)
    lp, sp, i1 = _host(c, 1e-4, "Huber", 0.01, 10, 1e-4)
    lp2, sp2, i2 = api.host_pose_graph_lm(lp, sp, c["edges"], i1["lambda_"])
    assert i2["trace"][0]["lambda_"] == i1["lambda_"]
    a = _literal(c, 1e-4, "Huber", 0.01, 10, 1e-4)
    b = PL.optimize(a[0], a[1], c["edges"], a[2], 10, 1e-4, "Huber", 0.01)
    _assert_same((lp2, sp2, i2), b)


@pytest.mark.parametrize("loss", PL.LOSSES)
def test_loss_and_weight_closed_forms(loss):
    s = 0.3
    for t in (0.0, 1e-3, 0.1, 0.3, 0.7, 5.0, 1e4):
        lo, w = api.host_pose_graph_loss(loss, s, t)
        if loss == "Squared":
            want = (t, 1.0)
        elif loss == "Huber":
            want = (t, 1.0) if t <= s else (2 * math.sqrt(s * t) - s, math.sqrt(s / t))
        elif loss == "Cauchy":
            want = (s * math.log(1 + t / s), 1 / (1 + t / s))
        elif loss == "Fair":
            q = math.sqrt(t / s)
            want = (2 * s * (q - math.log(1 + q)), 1 / (1 + q))
        elif loss == "GemanMcClure":
            want = (s * t / (s + t), 1 / (1 + t / s) ** 2)
        else:
            want = (s * (1 - math.exp(-t / s)), math.exp(-t / s))
        assert lo == pytest.approx(want[0], rel=1e-12, abs=1e-300)
        assert w == pytest.approx(want[1], rel=1e-12)
        assert (lo, w) == (PL.loss(loss, s, t), PL.weight(loss, s, t))


def _expect_einval(c, lam=1e-4, **kw):
    with pytest.raises(api.CsmError) as ex:
        api.host_pose_graph_lm(c["local"], c["scan"], c["edges"], lam, **kw)
    assert ex.value.code == L.CSM_EINVAL


def test_einval_paths():
    c = _case(22, 12, 4, 0.0, None)
    _expect_einval(c, solver="SparseCholesky")
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


def test_converged_step_solves_the_normal_equations():
    """One LM step: the CG's delta against numpy.linalg.solve on a dense copy of H and b"""
    c = _case(23, 30, 6, 0.1, None)
    lam = 1e-3
    H, b = PL.dense_system(c["local"].tolist(), c["scan"].tolist(), c["edges"], lam)
    assert np.array_equal(H, H.T)
    want = np.linalg.solve(H, b)
    lp, sp, info = _host(c, lam, "Huber", 0.01, 1, 1e-4)
    thr = (np.finfo(float).eps ** 2) * float(b @ b)
    assert info["trace"][0]["residual_norm2"] < thr     # converged, not capped
    got = np.concatenate([(lp - c["local"]).ravel(), (sp - c["scan"]).ravel()])
    scale = np.abs(want).max()
    assert np.abs(got - want).max() <= 1e-9 * scale + 1e-14, (np.abs(got - want).max(), scale)
