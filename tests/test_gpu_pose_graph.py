"""csm_pose_graph_lm (PoseGraphOptimizerLM::Optimize on the device) against the host restatement
csm_host_pose_graph_lm, which tests/test_cpu_pose_graph.py pins to the Python literal bit for bit.

The device reduces its dot products and the total error in a fixed tree instead of left to right,
and uses the device library's sin / cos, so it agrees with the host within rounding, not bit for bit.
The tolerances below were fixed before any GPU run, from the Python literal run sequentially and in
pairwise-tree order on the same kind of graphs (synth.pose_graph_case, 20 to 400 scan nodes, the
Squared, Huber, Cauchy and Welsch losses, with and without wrong loop edges):
  - poses:       max |sequential - pairwise| = 3.6e-15 (m / rad, poses of magnitude up to ~15);
                 POSE_ATOL = 1e-12 is ~300x that, for larger graphs and the 1-ulp sin / cos spread.
  - total error: max relative spread 7.4e-14 where the error is not ~0, 1e-17 absolute where it is;
                 TOTAL_RTOL = 1e-10 (~1000x), TOTAL_ATOL = 1e-12.
  - CG iterations: the count at which |r|^2 first falls below eps^2 |b|^2 moved by up to 127 of 734
                 (17 %); allowed: |device - host| <= 0.3 host + 8.
The LM decisions (number of steps, the lambda sequence) must agree exactly: every case asserts on
the host first that each decision's margin is at least DECISION_MARGIN times the total-error
tolerance, so a flip is a bug, not noise."""
import copy
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from csm_hip import _lib as L
from csm_hip import api, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "my-lidar-graph-slam-v2_amd", "host", "adapter_demo")
POSE_ATOL = 1e-12
TOTAL_RTOL, TOTAL_ATOL = 1e-10, 1e-12
DECISION_MARGIN = 100.0
LOSS_SCALE = {"Squared": 0.0, "Huber": 0.01, "Cauchy": 0.05, "Fair": 0.1, "GemanMcClure": 0.5, "Welsch": 1.0}


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


def _compare(dev, host, n_vars):
    dl, ds, di = dev
    hl, hs, hi = host
    assert di["steps"] == hi["steps"]
    assert [t["lambda_"] for t in di["trace"]] == [t["lambda_"] for t in hi["trace"]]
    assert di["lambda_"] == hi["lambda_"]
    assert np.abs(dl - hl).max() <= POSE_ATOL
    if len(hs):
        assert np.abs(ds - hs).max() <= POSE_ATOL, np.abs(ds - hs).max()
    assert abs(di["initial_error"] - hi["initial_error"]) <= _noise(hi["initial_error"])
    eps2 = np.finfo(float).eps ** 2
    for td, th in zip(di["trace"], hi["trace"]):
        assert abs(td["total_error"] - th["total_error"]) <= _noise(th["total_error"])
        assert abs(td["cg_iterations"] - th["cg_iterations"]) <= 0.3 * th["cg_iterations"] + 8
        assert 0 <= td["cg_iterations"] <= 2 * n_vars
    # each CG run ended on the stopping rule (or returned at once on b = 0), or on the 2n cap, as the host's did
    for t in di["trace"] + hi["trace"]:
        thr = max(eps2 * t["rhs_norm2"], np.finfo(float).tiny)
        assert t["cg_iterations"] == 2 * n_vars or t["residual_norm2"] < thr or t["rhs_norm2"] == 0.0


def _run_case(ctx, c, loss, lam=1e-4, tol=1e-4, itmax=10, scale=None):
    kw = dict(iterations_max=itmax, error_tolerance=tol, loss=loss,
              loss_scale=LOSS_SCALE[loss] if scale is None else scale)
    host = api.host_pose_graph_lm(c["local"], c["scan"], c["edges"], lam, **kw)
    _check_margins(host[2], tol)
    dev = ctx.pose_graph_lm(c["local"], c["scan"], c["edges"], lam, **kw)
    _compare(dev, host, 3 * (len(c["local"]) + len(c["scan"])))
    return dev, host


@pytest.mark.parametrize("loss", list(LOSS_SCALE))
@pytest.mark.parametrize("wrong", [0.0, 0.2])
def test_device_matches_host_each_loss(gpu_ctx, loss, wrong):
    c = synth.pose_graph_case(140, n_scans=100, wrong_fraction=wrong)
    assert any(e["loop"] for e in c["edges"])
    _run_case(gpu_ctx, c, loss)


# up to 1000 scan nodes: one launch stays under half a second (5000 take ~5 s on one workgroup;
# tools/bench_pose_graph.py compares the device with the host at 5000 and 10000)
@pytest.mark.parametrize("n,wrong", [(4, 0.0), (20, 0.2), (500, 0.1), (1000, 0.1)])
def test_device_matches_host_by_size(gpu_ctx, n, wrong):
    c = synth.pose_graph_case(40 + n, n_scans=n, wrong_fraction=wrong)
    _run_case(gpu_ctx, c, "Huber")


def test_device_is_deterministic(gpu_ctx):
    c = synth.pose_graph_case(540, n_scans=500, wrong_fraction=0.1)
    a = gpu_ctx.pose_graph_lm(c["local"], c["scan"], c["edges"], 1e-4)
    b = gpu_ctx.pose_graph_lm(c["local"], c["scan"], c["edges"], 1e-4)
    assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist()
    assert a[2] == b[2]


def test_robust_loss_rejects_wrong_loop_edges(gpu_ctx):
    c = synth.pose_graph_case(31, n_scans=300, wrong_fraction=0.3)
    assert len(c["wrong"]) >= 5
    err = {}
    for loss in ("Huber", "Squared"):
        lp, sp, _ = gpu_ctx.pose_graph_lm(c["local"], c["scan"], c["edges"], 1e-4, loss=loss,
                                          loss_scale=LOSS_SCALE[loss])
        err[loss] = np.abs(sp[:, :2] - c["truth_scan"][:, :2]).max()
        if loss == "Huber":
            nodes = np.concatenate([lp, sp])
            nl = len(lp)
            for k in c["wrong"]:
                e = c["edges"][k]
                ps, pe = nodes[e["local"]], nodes[nl + e["scan"]]
                s, co = np.sin(ps[2]), np.cos(ps[2])
                d = pe - ps
                ev = np.array([co * d[0] + s * d[1] - e["rel"][0], -s * d[0] + co * d[1] - e["rel"][1],
                               (d[2] - e["rel"][2] + np.pi) % (2 * np.pi) - np.pi])
                assert api.host_pose_graph_loss("Huber", 0.01, float(ev @ e["info"] @ ev))[1] < 0.1
    init = np.abs(c["scan"][:, :2] - c["truth_scan"][:, :2]).max()
    assert err["Huber"] < 0.6 * init, (err, init)
    assert err["Squared"] > 3.0 * err["Huber"], err


def test_python_optimizer_keeps_lambda_between_calls(gpu_ctx):
    c = synth.pose_graph_case(77, n_scans=60, wrong_fraction=0.1)
    opt = api.PoseGraphOptimizerLMHIP(ctx=gpu_ctx)
    lp, sp = opt.optimize(c["local"], c["scan"], c["edges"])
    first = opt.last_info
    assert opt.lambda_ == first["lambda_"] != 1e-4
    lp2, sp2 = opt.optimize(lp, sp, c["edges"])
    assert opt.last_info["trace"][0]["lambda_"] == first["lambda_"]
    h1 = api.host_pose_graph_lm(c["local"], c["scan"], c["edges"], 1e-4)
    h2 = api.host_pose_graph_lm(h1[0], h1[1], c["edges"], h1[2]["lambda_"])
    assert opt.lambda_ == h2[2]["lambda_"]
    assert np.abs(sp2 - h2[1]).max() <= POSE_ATOL
    with pytest.raises(api.CsmError):
        api.PoseGraphOptimizerLMHIP(solver="SparseCholesky", ctx=gpu_ctx)


def test_device_einval(gpu_ctx):
    c = synth.pose_graph_case(5, n_scans=12, scans_per_map=4)
    for kw, what in ((dict(solver="SparseCholesky"), "SparseCholesky"), (dict(iterations_max=0), "iterations_max")):
        with pytest.raises(api.CsmError) as ex:
            gpu_ctx.pose_graph_lm(c["local"], c["scan"], c["edges"], 1e-4, **kw)
        assert ex.value.code == L.CSM_EINVAL and what in str(ex.value)
    d = copy.deepcopy(c)
    d["edges"][1]["scan"] = 12
    with pytest.raises(api.CsmError) as ex:
        gpu_ctx.pose_graph_lm(d["local"], d["scan"], d["edges"], 1e-4)
    assert ex.value.code == L.CSM_EINVAL and "out of range" in str(ex.value)
    d = copy.deepcopy(c)
    d["scan"][3, 0] = float("nan")
    with pytest.raises(api.CsmError) as ex:
        gpu_ctx.pose_graph_lm(d["local"], d["scan"], d["edges"], 1e-4)
    assert ex.value.code == L.CSM_EINVAL and "non-finite" in str(ex.value)
    # the context still works afterwards
    _run_case(gpu_ctx, c, "Huber")


def test_cpp_pose_graph_optimizer_adapter(tmp_path):
    import __graft_entry__ as ge
    ge.build()
    c = synth.pose_graph_case(88, n_scans=80, wrong_fraction=0.1)
    ea = api.pose_graph_edges(c["edges"])
    p = str(tmp_path / "pg.bin")
    with open(p, "wb") as f:
        f.write(struct.pack("<6i", 5, len(c["local"]), len(c["scan"]), len(c["edges"]), 10, L.PG_LOSS_HUBER))
        f.write(struct.pack("<3d", 1e-4, 0.01, 1e-4))
        f.write(np.ascontiguousarray(c["local"]).tobytes())
        f.write(np.ascontiguousarray(c["scan"]).tobytes())
        f.write(bytes(ea))
    out = subprocess.run([DEMO, p], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    got = json.loads(out.stdout.strip().splitlines()[-1])
    assert got["cholesky_rejected"] == 1
    # the same two calls through the Python binding on a fresh context: the same device, the same bits
    ctx = api.Context(0)
    try:
        lp, sp, i1 = ctx.pose_graph_lm(c["local"], c["scan"], c["edges"], 1e-4)
        lp2, sp2, i2 = ctx.pose_graph_lm(lp, sp, c["edges"], i1["lambda_"])
    finally:
        ctx.close()
    for call, (l_, s_, info) in zip(got["calls"], ((lp, sp, i1), (lp2, sp2, i2))):
        assert float.fromhex(call["lambda"]) == info["lambda_"]
        assert call["steps"] == info["steps"]
        assert [float.fromhex(v) for v in call["poses"]] == np.concatenate([l_, s_]).ravel().tolist()
