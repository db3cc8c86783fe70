"""csm_pose_graph_lm with the direct Schur-complement Cholesky solver (CSM_PG_SOLVER_SCHUR_CHOLESKY) on the
device against the host restatement csm_host_pose_graph_lm with the same solver, which
tests/test_cpu_pose_graph_schur.py pins to the Python literal bit for bit.

The device subtracts every term of the Schur sums, of the LDL^T inner products and of the substitutions
in the host's order, but reduces |b|^2, the residual and the total error in a fixed tree and uses the
device library's sin / cos, so it agrees with the host within rounding. The tolerances are not those of
the conjugate-gradient test. They were fixed before any device run from the spread between the Python
literal (tests/pose_graph_schur_literal.py) in sequential order and in pairwise order (Schur sums, LDL^T
inner products, substitutions, norms, total error) on synth.pose_graph_case graphs of 20, 60, 150 and 400
scan nodes (seed 300 + n), all six losses, wrong loop fraction 0 and 0.2 (48 graphs; every pair of runs
took the same steps with the same lambdas):
  - poses:       max |sequential - pairwise| = 7.276401703393276e-13 (400 scan nodes, Welsch);
                 POSE_ATOL = 300x that = 2.18e-10, for larger graphs and the 1-ulp sin / cos spread.
  - total error: max relative spread 6.603568874741998e-13 where the error is not ~0 (|total| > 1e-9),
                 7.899575007653595e-23 absolute where it is; TOTAL_RTOL and TOTAL_ATOL are 1000x those.
  - residual_norm2: on the twenty graphs of the CPU test, at most ten times the CPU test's bound, which
                 is ten times the largest residual_norm2 / rhs_norm2 of the Python literal on those
                 graphs (9.063279157428158e-27). Larger graphs have larger ratios in the literal too
                 (2.7e-24 at 400 scan nodes), so the other tests print the ratio and do not bound it.
The LM decisions (number of steps, the lambda sequence) must agree exactly: every case asserts on the
host first that each decision's margin is at least DECISION_MARGIN times the total-error tolerance."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from csm_hip import _lib as L
from csm_hip import api, synth
from test_cpu_pose_graph import CASES, _case
from test_cpu_pose_graph_schur import RESIDUAL_RATIO_BOUND

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "my-lidar-graph-slam-v2_amd", "host", "adapter_demo")
POSE_ATOL = 300.0 * 7.276401703393276e-13
TOTAL_RTOL, TOTAL_ATOL = 1000.0 * 6.603568874741998e-13, 1000.0 * 7.899575007653595e-23
DECISION_MARGIN = 100.0
LOSS_SCALE = {"Squared": 0.0, "Huber": 0.01, "Cauchy": 0.05, "Fair": 0.1, "GemanMcClure": 0.5, "Welsch": 1.0}
SOLVER = "SchurCholesky"
SMALL = 96       # 3 n_local up to here: one workgroup, S in LDS; above: the blocked factorization
TILE = 48        # its panel width


def _noise(total):
    return TOTAL_RTOL * abs(total) + TOTAL_ATOL


def _check_margins(info, tol):
    prev = 1.7976931348623157e308
    for t in info["trace"]:
        tot = t["total_error"]
        d = abs(prev - tot)
        assert abs(d - tol) >= DECISION_MARGIN * _noise(tot), "case too close to the stop decision"
        if d >= tol:
            assert abs(tot - prev) >= DECISION_MARGIN * _noise(tot), "case too close to the lambda decision"
        prev = tot


def _compare(dev, host):
    dl, ds, di = dev
    hl, hs, hi = host
    assert di["steps"] == hi["steps"]
    assert [t["lambda_"] for t in di["trace"]] == [t["lambda_"] for t in hi["trace"]]
    assert di["lambda_"] == hi["lambda_"]
    pose = max(np.abs(dl - hl).max(), np.abs(ds - hs).max() if len(hs) else 0.0)
    print("max pose difference", pose)
    assert pose <= POSE_ATOL, pose
    assert abs(di["initial_error"] - hi["initial_error"]) <= _noise(hi["initial_error"])
    assert abs(di["final_error"] - hi["final_error"]) <= _noise(hi["final_error"])
    assert di["cg_iterations"] == 0
    for td, th in zip(di["trace"], hi["trace"]):
        print("total", td["total_error"], th["total_error"], "residual ratio",
              td["residual_norm2"] / td["rhs_norm2"] if td["rhs_norm2"] else 0.0)
        assert abs(td["total_error"] - th["total_error"]) <= _noise(th["total_error"])
        assert td["cg_iterations"] == 0
        assert abs(td["rhs_norm2"] - th["rhs_norm2"]) <= 1e-6 * th["rhs_norm2"]


def _run_case(ctx, c, loss, lam=1e-4, tol=1e-4, itmax=10):
    kw = dict(iterations_max=itmax, error_tolerance=tol, loss=loss, loss_scale=LOSS_SCALE[loss], solver=SOLVER)
    host = api.host_pose_graph_lm(c["local"], c["scan"], c["edges"], lam, **kw)
    _check_margins(host[2], tol)
    dev = ctx.pose_graph_lm(c["local"], c["scan"], c["edges"], lam, **kw)
    _compare(dev, host)
    return dev, host


@pytest.mark.parametrize("loss", list(LOSS_SCALE))
@pytest.mark.parametrize("wrong", [0.0, 0.2])
def test_schur_device_matches_host_each_loss(gpu_ctx, loss, wrong):
    # seed 141: with 140 (the conjugate-gradient test's) the Squared / 0.2 case lacks the decision margin
    c = synth.pose_graph_case(141, n_scans=100, wrong_fraction=wrong)
    assert any(e["loop"] for e in c["edges"])
    _run_case(gpu_ctx, c, loss)


@pytest.mark.parametrize("n,wrong", [(4, 0.0), (20, 0.2), (500, 0.1), (1000, 0.1), (5000, 0.1)])
def test_schur_device_matches_host_by_size(gpu_ctx, n, wrong):
    c = synth.pose_graph_case(40 + n, n_scans=n, wrong_fraction=wrong)
    _run_case(gpu_ctx, c, "Huber")


# n_local 31 / 32 / 33: 3 n_local one block below, at and above the switch to the blocked
# factorization; 34, 47, 49, 70: 3 n_local = 102, 141, 147, 210, no multiples of the panel width
# (48 = 144 is one: 3 tiles exactly), so the last tile is padded
@pytest.mark.parametrize("n_local", [31, 32, 33, 34, 47, 48, 49, 70])
def test_schur_single_workgroup_and_blocked_paths(gpu_ctx, n_local):
    assert (3 * n_local <= SMALL) == (n_local <= 32)
    c = synth.pose_graph_case(700 + n_local, n_scans=10 * n_local, wrong_fraction=0.1)
    assert len(c["local"]) == n_local
    _run_case(gpu_ctx, c, "Huber")


@pytest.mark.parametrize("case", CASES, ids=[str(c[0]) for c in CASES])
def test_schur_device_residual(gpu_ctx, case):
    seed, n, spm, wf, loss, scale, itmax, tol, lam, variant = case
    c = _case(seed, n, spm, wf, variant)
    _, _, info = gpu_ctx.pose_graph_lm(c["local"], c["scan"], c["edges"], lam, iterations_max=itmax,
                                       error_tolerance=tol, loss=loss, loss_scale=scale, solver=SOLVER)
    for t in info["trace"]:
        print("device ratio", t["residual_norm2"] / t["rhs_norm2"] if t["rhs_norm2"] else 0.0)
        assert t["residual_norm2"] <= 10.0 * RESIDUAL_RATIO_BOUND * t["rhs_norm2"]
        assert t["cg_iterations"] == 0


@pytest.mark.parametrize("n", [100, 500, 1500])
def test_schur_device_is_deterministic(gpu_ctx, n):
    c = synth.pose_graph_case(540, n_scans=n, wrong_fraction=0.1)
    a = gpu_ctx.pose_graph_lm(c["local"], c["scan"], c["edges"], 1e-4, solver=SOLVER)
    b = gpu_ctx.pose_graph_lm(c["local"], c["scan"], c["edges"], 1e-4, solver=SOLVER)
    assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist()
    assert a[2] == b[2]


def test_schur_between_two_conjugate_gradient_calls_and_memory():
    """CG, direct, CG on one context: the two CG results are equal bit for bit, and the context gives
    back every byte (the dense Schur complement included) when it is closed."""
    lib = L.load()
    import ctypes as C
    d0, p0 = C.c_int64(), C.c_int64()
    assert lib.csm_debug_live_bytes(C.byref(d0), C.byref(p0)) == 0
    c = synth.pose_graph_case(91, n_scans=600, wrong_fraction=0.1)
    s = synth.pose_graph_case(92, n_scans=60, wrong_fraction=0.1)
    ctx = api.Context(0)
    try:
        a = ctx.pose_graph_lm(c["local"], c["scan"], c["edges"], 1e-4)
        m = ctx.pose_graph_lm(c["local"], c["scan"], c["edges"], 1e-4, solver=SOLVER)
        ctx.pose_graph_lm(s["local"], s["scan"], s["edges"], 1e-4, solver=SOLVER)
        b = ctx.pose_graph_lm(c["local"], c["scan"], c["edges"], 1e-4)
        d1, p1 = C.c_int64(), C.c_int64()
        lib.csm_debug_live_bytes(C.byref(d1), C.byref(p1))
        assert d1.value - d0.value >= 8 * (3 * len(c["local"])) ** 2
    finally:
        ctx.close()
    assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist() and a[2] == b[2]
    assert m[2]["cg_iterations"] == 0 and a[2]["cg_iterations"] > 0
    d2, p2 = C.c_int64(), C.c_int64()
    lib.csm_debug_live_bytes(C.byref(d2), C.byref(p2))
    assert (d2.value, p2.value) == (d0.value, p0.value)


def test_schur_python_optimizer_keeps_lambda_between_calls(gpu_ctx):
    c = synth.pose_graph_case(77, n_scans=60, wrong_fraction=0.1)
    opt = api.PoseGraphOptimizerLMHIP(solver=SOLVER, ctx=gpu_ctx)
    assert opt.params.solver_type == L.PG_SOLVER_SCHUR_CHOLESKY == api.PG_SOLVERS[SOLVER] == 2
    lp, sp = opt.optimize(c["local"], c["scan"], c["edges"])
    first = opt.last_info
    assert opt.lambda_ == first["lambda_"] != 1e-4
    lp2, sp2 = opt.optimize(lp, sp, c["edges"])
    assert opt.last_info["trace"][0]["lambda_"] == first["lambda_"]
    h1 = api.host_pose_graph_lm(c["local"], c["scan"], c["edges"], 1e-4, solver=SOLVER)
    h2 = api.host_pose_graph_lm(h1[0], h1[1], c["edges"], h1[2]["lambda_"], solver=SOLVER)
    assert opt.lambda_ == h2[2]["lambda_"]
    assert np.abs(sp2 - h2[1]).max() <= POSE_ATOL
    assert api.PoseGraphOptimizerLMHIP(ctx=gpu_ctx).params.solver_type == L.PG_SOLVER_CONJUGATE_GRADIENT


def test_schur_device_einval(gpu_ctx):
    lib = L.load()
    import ctypes as C
    d0, p0 = C.c_int64(), C.c_int64()
    lib.csm_debug_live_bytes(C.byref(d0), C.byref(p0))
    big_local = np.zeros((L.PG_SCHUR_MAX_LOCAL + 1, 3))
    edges = [dict(local=0, scan=0, rel=[0.0, 0.0, 0.0], info=np.eye(3), loop=False)]
    with pytest.raises(api.CsmError) as ex:
        gpu_ctx.pose_graph_lm(big_local, np.zeros((1, 3)), edges, 1e-4, solver=SOLVER)
    assert ex.value.code == L.CSM_EINVAL and "n_local" in str(ex.value)
    d1, p1 = C.c_int64(), C.c_int64()
    lib.csm_debug_live_bytes(C.byref(d1), C.byref(p1))
    assert d1.value == d0.value           # nothing was allocated for the refused call
    c = synth.pose_graph_case(5, n_scans=12, scans_per_map=4)
    with pytest.raises(api.CsmError) as ex:
        gpu_ctx.pose_graph_lm(c["local"], c["scan"], c["edges"], 1e-4, solver=SOLVER, iterations_max=0)
    assert ex.value.code == L.CSM_EINVAL and "iterations_max" in str(ex.value)
    with pytest.raises(api.CsmError) as ex:
        gpu_ctx.pose_graph_lm(c["local"], c["scan"], c["edges"], 1e-4, solver=3)
    assert ex.value.code == L.CSM_EINVAL and "unknown solver" in str(ex.value)
    _run_case(gpu_ctx, c, "Huber")


def test_schur_cpp_adapter_gives_the_python_binding_s_bits(tmp_path):
    import __graft_entry__ as ge
    ge.build()
    c = synth.pose_graph_case(88, n_scans=80, wrong_fraction=0.1)
    ea = api.pose_graph_edges(c["edges"])
    p = str(tmp_path / "pg.bin")
    with open(p, "wb") as f:
        f.write(struct.pack("<6i", 6, len(c["local"]), len(c["scan"]), len(c["edges"]), 10, L.PG_LOSS_HUBER))
        f.write(struct.pack("<3d", 1e-4, 0.01, 1e-4))
        f.write(np.ascontiguousarray(c["local"]).tobytes())
        f.write(np.ascontiguousarray(c["scan"]).tobytes())
        f.write(bytes(ea))
    out = subprocess.run([DEMO, p], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    got = json.loads(out.stdout.strip().splitlines()[-1])
    assert got["cholesky_rejected"] == 1
    ctx = api.Context(0)
    try:
        lp, sp, i1 = ctx.pose_graph_lm(c["local"], c["scan"], c["edges"], 1e-4, solver=SOLVER)
        lp2, sp2, i2 = ctx.pose_graph_lm(lp, sp, c["edges"], i1["lambda_"], solver=SOLVER)
    finally:
        ctx.close()
    for call, (l_, s_, info) in zip(got["calls"], ((lp, sp, i1), (lp2, sp2, i2))):
        assert float.fromhex(call["lambda"]) == info["lambda_"]
        assert call["steps"] == info["steps"]
        assert [float.fromhex(v) for v in call["poses"]] == np.concatenate([l_, s_]).ravel().tolist()
