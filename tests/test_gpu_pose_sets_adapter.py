"""The pose sets through the C++ host side and the Python methods: host/adapter_demo's mode 7
(ScorePixelAccurateHIP::Score / ScoreManyRobotPoses and ParticleSetHIP::MeasurementUpdate on one context) and
Context.score_pixel_accurate / score_pixel_accurate_many / measurement_update, against the literal Python of
tests/pose_set_reference.py and the oracle's ScorePixelAccurate."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import pose_set_reference as R
from csm_hip import api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "my-lidar-graph-slam-v2_amd", "host", "adapter_demo")

REL = (0.11, -0.04, 0.07)
TEMPERATURE, THRESHOLD, N_OUT, OFFSET = 0.04, 0.2, 90, 0xFEDCBA9876543210


@pytest.fixture(scope="module")
def case():
    grid = R.make_map(7)
    angles, ranges = R.make_scan(7, 65, 0.2, 1.0)
    robot = R.make_poses(7, 70, 0.8, 0.6)
    sensor = np.array([api.host_compound(p, REL) for p in robot])
    S, K = R.score_poses(grid, R.GEOM, angles, ranges, sensor)
    want = R.update(S.tolist(), K.tolist(), 65, TEMPERATURE, THRESHOLD, N_OUT, OFFSET)
    return dict(grid=grid, angles=angles, ranges=ranges, robot=robot, sensor=sensor, S=S, K=K, want=want)


def _ess(weights):
    w = np.asarray(weights, np.float64)
    return float(w.sum()) ** 2 / float((w * w).sum())


def test_cpp_adapters(tmp_path, case):
    path = str(tmp_path / "poses.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<6i", 7, R.ROWS, R.COLS, 65, len(case["robot"]), N_OUT))
        f.write(struct.pack("<8d", *R.GEOM, TEMPERATURE, float(OFFSET & 0xFFFFFFFF), float(OFFSET >> 32), 0.0, THRESHOLD))
        f.write(struct.pack("<3d", *REL))
        f.write(case["robot"].tobytes())
        f.write(case["angles"].tobytes())
        f.write(case["ranges"].tobytes())
        f.write(case["grid"].tobytes())
    assert os.path.exists(DEMO), "host/adapter_demo is built by __graft_entry__.build()"
    run = subprocess.run([DEMO, path], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr + run.stdout
    got = json.loads(run.stdout.strip().splitlines()[-1])
    w, a, upd = case["want"]
    rows = [got["one"]] + got["all"]
    for row, p in zip(rows, [0] + list(range(len(case["robot"])))):
        score, rate = api.host_score_from_sums(case["S"][p], case["K"][p], 65)
        assert row[:2] == [case["S"][p], case["K"][p]], p
        assert [float.fromhex(v) for v in row[2:]] == [score, score * 65.0, rate]
    assert len(got["all"]) == len(case["robot"])
    assert got["weights"] == w and got["ancestors"] == a
    assert {k: got[k] for k in upd} == upd
    assert float.fromhex(got["ess"]) == _ess(w)
    assert got["uncertain"] == 0


def test_python_methods(gpu_ctx, oracle, case):
    mid = 9200
    gpu_ctx.upload_grid(mid, case["grid"])
    try:
        many = gpu_ctx.score_pixel_accurate_many(mid, R.GEOM, case["angles"], case["ranges"], case["robot"], rel_pose=REL)
        direct = gpu_ctx.score_pixel_accurate_many(mid, R.GEOM, case["angles"], case["ranges"], case["sensor"])
        assert many == direct and len(many) == len(case["robot"])
        for p, m in enumerate(many):
            want, known = oracle.score_at(case["grid"], R.GEOM, case["angles"], case["ranges"], case["sensor"][p])
            assert (m["sum_values"], m["known"]) == (case["S"][p], case["K"][p])
            assert abs(m["normalized_score"] - want) <= 1e-12 and m["known_rate"] == known / 65
            assert m["score"] == m["normalized_score"] * 65
        assert gpu_ctx.score_pixel_accurate(mid, R.GEOM, case["angles"], case["ranges"], case["robot"][3], REL) == many[3]
        out = gpu_ctx.measurement_update(mid, R.GEOM, case["angles"], case["ranges"], case["robot"], TEMPERATURE,
                                         THRESHOLD, N_OUT, OFFSET, rel_pose=REL)
        w, a, upd = case["want"]
        assert out["weights"].tolist() == w and out["ancestors"].tolist() == a and out["update"] == upd
        assert out["effective_sample_size"] == _ess(w)
        assert np.array_equal(out["records"]["sum_values"], case["S"])
    finally:
        gpu_ctx.release_grid(mid)
