"""The library's host restatements of the greedy-endpoint cost and the
hill-climbing matcher (csm_host_greedy_cost, csm_host_hill_climbing) against the
Python literal (tests/greedy_literal.py), bit for bit. CPU only: these are the
fallback of the device path and the reference the GPU tests lean on for large
batches. The settings (CASES) are shared with tests/test_gpu_greedy_edges.py through
tests/greedy_edge_cases.py."""
import math

import numpy as np
import pytest

from csm_hip import api
import cost_edge_cases as GE_cost
import greedy_edge_cases as GE
from greedy_edge_cases import CASES, case as _case
import greedy_literal as GL


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
    prm = GE.settings(greedy)
    lit = GL.Greedy(**prm)
    sensor = tuple(api.host_compound(init, c["rel_pose"]))
    got, cov = api.host_greedy_cost(grid, c["geom"], c["angles"], c["ranges"], sensor, prm, covariance=True)
    want = lit.cost(grid, c["geom"], c["angles"], c["ranges"], sensor)
    assert got == want
    assert np.array_equal(cov, lit.covariance(grid, c["geom"], c["angles"], c["ranges"], sensor), equal_nan=True)


@pytest.mark.parametrize("seed,greedy,hc,opts", CASES)
def test_host_hill_climbing_bit_exact(seed, greedy, hc, opts):
    grid, c, init = _case(seed, **opts)
    prm = GE.settings(greedy)
    got = api.host_hill_climbing(grid, c["geom"], c["angles"], c["ranges"], c["rel_pose"], init,
                                 *hc, greedy=prm)
    want = GL.optimize_pose(grid, c["geom"], c["angles"], c["ranges"], c["rel_pose"], init, *hc, prm)
    for key in ("normalized_initial_cost", "normalized_cost", "sensor_pose", "best_sensor_pose",
                "estimated_pose", "iterations", "refinements", "diff_translation", "diff_rotation"):
        assert got[key] == want[key], key
    assert np.array_equal(got["covariance"], want["covariance"], equal_nan=True)
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


def _row(seed):
    return next(r for r in CASES if r[0] == seed)


def test_sweep_rows_reach_their_edges():
    """The rows of CASES added for the device sweep are what they claim to be."""
    pl = GL.plut()
    # the threshold rows: a planted value under hit and missed points, exactly the threshold
    for seed in (24, 25, 27):
        _, greedy, _, opts = _row(seed)
        grid, c, init = _case(seed, **opts)
        prm = GE.settings(greedy)
        v = opts["plant"]
        assert pl[v] == prm["occupancy_threshold"] and (pl[1:] == pl[v]).sum() == 1
        sensor = tuple(api.host_compound(init, c["rel_pose"]))
        idx = GE.cell_indices(c["geom"], sensor, c["angles"], c["ranges"], prm["hit_and_missed_dist"])
        for kind in ("hit", "missed"):
            col, row = idx[kind]
            inside = (row >= 0) & (row < grid.shape[0]) & (col >= 0) & (col < grid.shape[1])
            assert (grid[row[inside], col[inside]] == v).sum() >= 3, (seed, kind)
    assert _row(26)[1]["occupancy_threshold"] < pl[1] and _row(28)[1]["occupancy_threshold"] > pl[65535]
    # denormal / -0.0 tables, with the denormal ones negative and nonzero
    for seed in (29, 30):
        lit = GL.Greedy(**GE.settings(_row(seed)[1]))
        vals = np.array(lit.lut + [lit.default])
        denormal = (vals != 0.0) & (np.abs(vals) < np.finfo(np.float64).tiny)
        neg_zero = (vals == 0.0) & np.signbit(vals)
        assert denormal.sum() == 4 and neg_zero.sum() + denormal.sum() >= len(vals) // 2
        assert lit.default == 0.0 and np.signbit(lit.default)
    assert len(set(GL.Greedy(**GE.settings(_row(31)[1])).lut)) == 1
    # missed points behind the sensor
    _, c, _ = _case(32, **_row(32)[3])
    hmd = _row(32)[1]["hit_and_missed_dist"]
    assert (c["ranges"] < hmd).any() and (c["ranges"] > hmd).any()
    # costs overflow to -inf: everywhere with 180 beams, at some poses only with two
    for seed in (36, 37):
        _, greedy, _, opts = _row(seed)
        grid, c, init = _case(seed, **opts)
        sensor = tuple(api.host_compound(init, c["rel_pose"]))
        lit = GL.Greedy(**GE.settings(greedy))
        cost = lit.cost(grid, c["geom"], c["angles"], c["ranges"], sensor)
        assert cost == -math.inf if seed == 36 else math.isfinite(cost)


def test_literal_alloc_reads_unknown():
    """Greedy.beam_values(alloc=): a read in an unallocated block is 0.0, as if the cell were
    unknown; a bitmap with every block allocated changes nothing."""
    grid, c, init = _case(3)
    sensor = tuple(api.host_compound(init, c["rel_pose"]))
    lit = GL.Greedy(**GE.settings(dict(kernel_size=2)))
    args = (c["geom"], c["angles"], c["ranges"], sensor)
    full = np.ones((-(-grid.shape[0] // 8), -(-grid.shape[1] // 8)), np.uint8)
    assert np.array_equal(lit.beam_values(grid, *args, alloc=(full, 3)), lit.beam_values(grid, *args))
    mask = (np.random.RandomState(3).rand(*full.shape) < 0.6).astype(np.uint8)
    zeroed = grid * np.kron(mask, np.ones((8, 8), np.uint16))[:grid.shape[0], :grid.shape[1]]
    a = lit.beam_values(grid, *args, alloc=(mask, 3))
    assert np.array_equal(a, lit.beam_values(zeroed, *args))
    assert not np.array_equal(a, lit.beam_values(grid, *args))


def _oracle_replays(oracle):
    for log2_block in (3, 4, 5):
        w = GE_cost.fresh_construct(oracle, log2_block)
        yield "fresh", log2_block, w["grid"], w["alloc"], w["queries"]
    for f in GE_cost.frontend_frames(oracle, 4):
        if f["k"] % 6 == 1:
            yield "frontend", 4, f["grid"], f["alloc"], [f["query"]]
    for s in GE_cost.local_map_steps(oracle, 3):
        if s["query"] is not None:
            yield "local", 3, s["grid"], s["alloc"], [s["query"]]


def test_device_built_maps_hold_known_cells_only_in_allocated_blocks(oracle):
    """What "unallocated blocks read 0, so the device needs no bitmap" rests on: in the oracle's
    replays of device-built maps (the inputs of test_gpu_greedy_edges.py), every nonzero cell lies
    in an allocated block, so the literal reads the same with and without the tracked bitmap."""
    lit = GL.Greedy(**GE.settings(dict(kernel_size=3)))
    reads = 0
    for kind, log2_block, grid, alloc, queries in _oracle_replays(oracle):
        bs = 1 << log2_block
        assert alloc.shape == (-(-grid.shape[0] // bs), -(-grid.shape[1] // bs))
        known = oracle.derived_alloc(grid, log2_block)
        assert not (known & ~alloc).any(), kind
        q = queries[0]
        sensor = tuple(api.host_compound(q["init_pose"], q["rel_pose"]))
        args = (q["geom"], q["angles"], q["ranges"], sensor)
        assert np.array_equal(lit.beam_values(grid, *args, alloc=(alloc, log2_block)), lit.beam_values(grid, *args))
        reads += GE.window_reads(grid, alloc, log2_block, q["geom"], sensor, q["angles"], q["ranges"], 3,
                                 GL.DEFAULT_GREEDY["hit_and_missed_dist"])[0]
    assert reads > 0         # the windows do reach unallocated blocks


def test_edge_queries_are_built_exactly():
    """The host-fallback queries of test_gpu_greedy_edges.py: a hit coordinate exactly on a cell
    edge at the start, or at the first +x candidate only; the host restatement equals the literal
    on them."""
    grid, geom, segs = GE.edge_map(61)
    hc = (GE.EDGE_STEP, 0.05, 10, 2)
    for start in (GE.start_on_edge(), GE.first_move_on_edge()):
        angles, ranges = GE.edge_scan(segs, start, 360)
        assert angles[0] == 0.0 and ranges[0] == 2.5
        got = api.host_hill_climbing(grid, geom, angles, ranges, (0.0, 0.0, 0.0), start, *hc,
                                     greedy=GL.DEFAULT_GREEDY)
        want = GL.optimize_pose(grid, geom, angles, ranges, (0.0, 0.0, 0.0), start, *hc, None)
        for key in ("normalized_initial_cost", "normalized_cost", "best_sensor_pose", "iterations",
                    "refinements"):
            assert got[key] == want[key], key
        assert np.array_equal(got["covariance"], want["covariance"])
