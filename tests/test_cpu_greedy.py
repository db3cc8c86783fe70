"""The library's host restatements of the greedy-endpoint cost and the
hill-climbing matcher (csm_host_greedy_cost, csm_host_hill_climbing) against the
Python literal (tests/greedy_literal.py), bit for bit. CPU only: these are the
fallback of the device path and the reference the GPU tests lean on for large
batches."""
import math

import numpy as np
import pytest

from csm_hip import api, synth
import greedy_literal as GL


def _case(seed, n_beams=180, unknown=False, off_map=False, res=0.05):
    c = synth.csm_case(seed, rows=200, cols=220, res=res, n_beams=n_beams, fov=1.5 * math.pi,
                       max_range=4.0, rel_pose=(0.05, -0.02, 0.01))
    grid = c["grid"].copy()
    if unknown:
        grid[60:140, :90] = 0            # an unknown region under part of the scan
    init = tuple(c["init_pose"])
    if off_map == "partly":
        init = (init[0] + 0.45 * grid.shape[1] * res, init[1], init[2])
    elif off_map == "wholly":
        init = (init[0] + 40.0, init[1] - 40.0, init[2])
    return grid, c, init


CASES = [
    # (seed, greedy overrides, hill-climbing settings, case options)
    (1, dict(kernel_size=0), (0.1, 0.1, 100, 5), {}),
    (2, dict(kernel_size=1), (0.1, 0.1, 100, 5), {}),
    (3, dict(kernel_size=2), (0.1, 0.1, 100, 5), {}),
    (4, dict(kernel_size=3), (0.05, 0.05, 30, 3), {}),
    (5, dict(occupancy_threshold=0.6), (0.1, 0.1, 100, 5), {}),
    (6, dict(occupancy_threshold=0.6, kernel_size=2), (0.01, 0.01, 5, 2), {}),
    (7, dict(scaling_factor=2.5), (0.1, 0.1, 100, 5), {}),
    (8, dict(scaling_factor=-1.0), (0.1, 0.1, 20, 5), {}),
    (9, dict(map_resolution=0.03), (0.1, 0.1, 100, 5), {}),
    (10, dict(map_resolution=0.08, kernel_size=2), (0.01, 0.01, 5, 2), {}),
    (11, {}, (0.1, 0.1, 100, 5), dict(off_map="partly")),
    (12, {}, (0.1, 0.1, 100, 5), dict(off_map="wholly")),
    (13, {}, (0.1, 0.1, 100, 5), dict(unknown=True)),
    (14, dict(kernel_size=2), (0.1, 0.1, 1, 5), {}),
    (15, {}, (0.1, 0.1, 100, 0), {}),
    (16, {}, (0.01, 0.01, 5, 2), {}),
    (17, dict(hit_and_missed_dist=0.15, standard_deviation=0.1), (0.1, 0.1, 100, 5), {}),
    (18, {}, (0.1, 0.1, 100, 5), dict(res=0.04)),
    (19, dict(scaling_factor=2.5, kernel_size=0), (0.05, 0.1, 40, 1), dict(unknown=True)),
    (20, dict(kernel_size=1), (0.1, 0.1, 100, 5), dict(n_beams=2)),
]


def test_lut_and_default_closed_form():
    for res, k, sd in [(0.05, 1, 0.05), (0.03, 3, 0.07), (0.1, 0, 0.02), (0.05, 8, 0.05)]:
        g = GL.Greedy(res, 0.075, 0.1, k, sd, 1.0)
        size = 2 * k + 1
        for ky in range(-k, k + 1):
            for kx in range(-k, k + 1):
                d2 = (res * kx) ** 2 + (res * ky) ** 2
                want = -math.exp(-0.5 * d2 / (sd * sd))
                assert g.lut[(k + ky) * size + k + kx] == pytest.approx(want, rel=1e-15, abs=1e-300)
        d2 = 2 * (res * (k + 1)) ** 2
        assert g.default == pytest.approx(-math.exp(-0.5 * d2 / (sd * sd)), rel=1e-15)
        assert g.lut[k * size + k] == -1.0
        assert max(g.lut) <= g.default


@pytest.mark.parametrize("seed,greedy,hc,opts", CASES)
def test_host_greedy_cost_bit_exact(seed, greedy, hc, opts):
    grid, c, init = _case(seed, **opts)
    prm = {**GL.DEFAULT_GREEDY, **greedy}
    lit = GL.Greedy(**prm)
    sensor = tuple(api.host_compound(init, c["rel_pose"]))
    got, cov = api.host_greedy_cost(grid, c["geom"], c["angles"], c["ranges"], sensor, prm, covariance=True)
    want = lit.cost(grid, c["geom"], c["angles"], c["ranges"], sensor)
    assert got == want
    assert np.array_equal(cov, lit.covariance(grid, c["geom"], c["angles"], c["ranges"], sensor))


@pytest.mark.parametrize("seed,greedy,hc,opts", CASES)
def test_host_hill_climbing_bit_exact(seed, greedy, hc, opts):
    grid, c, init = _case(seed, **opts)
    prm = {**GL.DEFAULT_GREEDY, **greedy}
    got = api.host_hill_climbing(grid, c["geom"], c["angles"], c["ranges"], c["rel_pose"], init,
                                 *hc, greedy=prm)
    want = GL.optimize_pose(grid, c["geom"], c["angles"], c["ranges"], c["rel_pose"], init, *hc, prm)
    for key in ("normalized_initial_cost", "normalized_cost", "sensor_pose", "best_sensor_pose",
                "estimated_pose", "iterations", "refinements", "diff_translation", "diff_rotation"):
        assert got[key] == want[key], key
    assert np.array_equal(got["covariance"], want["covariance"])
    assert got["iterations"] <= hc[2]
    if opts.get("off_map") == "wholly":
        # every beam reads the default: no move improves, the search ends by refinements
        assert got["refinements"] == hc[3] and got["best_sensor_pose"] == got["sensor_pose"]


def test_host_entries_reject_bad_parameters():
    grid, c, init = _case(1)
    a, r = c["angles"], c["ranges"]
    for bad in [dict(kernel_size=-1), dict(kernel_size=9), dict(standard_deviation=0.0),
                dict(standard_deviation=-1.0)]:
        with pytest.raises(api.CsmError) as e:
            api.host_greedy_cost(grid, c["geom"], a, r, init, {**GL.DEFAULT_GREEDY, **bad})
        assert e.value.code == api.L.CSM_EINVAL
    for hc in [(0.0, 0.1, 10, 1), (0.1, -0.1, 10, 1), (0.1, 0.1, 0, 1)]:
        with pytest.raises(api.CsmError) as e:
            api.host_hill_climbing(grid, c["geom"], a, r, c["rel_pose"], init, *hc)
        assert e.value.code == api.L.CSM_EINVAL
    with pytest.raises(api.CsmError) as e:
        api.host_hill_climbing(grid, c["geom"], a[:0], r[:0], c["rel_pose"], init)
    assert e.value.code == api.L.CSM_EINVAL
