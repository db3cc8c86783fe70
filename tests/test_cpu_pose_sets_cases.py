"""CPU side of the pose sets' second round: every condition tests/test_gpu_pose_sets_edges.py relies on is proven
here without a GPU. The constructed records of the cell-picking cases equal the host restatement
(csm_host_score_poses) and the literal (pose_set_reference.score_poses over the oracle's projection); the
certificate's margin in numpy marks no cell-picking pose, every forced pose and at most 1 % of each generic
case; update_fast equals the definition update(); csm_host_pose_set_update equals update_fast on every update
case, the 2^18 ones included; and the host entry refuses 65537 beams."""
import numpy as np
import pytest

import pose_set_cases as PC
import pose_set_reference as R
from csm_hip import _lib as L
from csm_hip import api
from test_cpu_pose_sets import _host_score_rc


def _picking_cases():
    yield "eligibility", PC.eligibility_case()
    for n in PC.TILE_SHAPES:
        yield "tile_%d" % n, PC.tile_shape_case(n)
    for first in PC.TIE_FIRST:
        yield "tie_%d" % first, PC.tie_case(first)
    for layout in PC.ZERO_LAYOUTS:
        yield "zeros_" + layout, PC.zero_runs_case(layout)
    yield "limit", PC.limit_case(False)
    yield "limit_unique_last", PC.limit_case(True)


def _records(S, K):
    rec = np.zeros(len(S), api.POSE_RECORD)
    rec["sum_values"], rec["known"] = S, K
    return rec


def _assert_host_is_fast(c, temperature, threshold=0.0, n_out=None, offset=0):
    want = R.update_fast(c["S"].tolist(), c["K"].tolist(), c["n_points"], temperature, threshold, n_out, offset)
    w, a, info = api.host_pose_set_update(_records(c["S"], c["K"]), c["n_points"], temperature, threshold, n_out,
                                          offset)
    assert w.tolist() == want[0] and a.tolist() == want[1] and info == want[2]
    return want


def test_cell_picking_records_are_the_constructed_ones(oracle):
    for name, c in _picking_cases():
        n = c["poses"].shape[0]
        assert c["grid"].shape == (PC.ROWS, PC.COLS) and not c["poses"][:, 2].any() and not c["angles"].any()
        rec = api.host_score_poses(c["grid"], c["geom"], c["angles"], c["ranges"], c["poses"])
        got_s, got_k = R.records_sk(rec)
        assert np.array_equal(got_s, c["S"]) and np.array_equal(got_k, c["K"]), name
        assert not rec["flags"].any()
        pick = np.arange(n)
        if n > 4000:                                     # first, last and 256 seeded poses through the literal
            pick = np.unique(np.concatenate([[0, n - 1], np.random.RandomState(n).randint(0, n, 256)]))
        S, K = R.score_poses(c["grid"], c["geom"], c["angles"], c["ranges"], c["poses"][pick])
        assert np.array_equal(S, c["S"][pick]) and np.array_equal(K, c["K"][pick]), name
        distinct = np.unique(c["poses"], axis=0)         # poses on the same cell are the same pose
        assert not R.margin_uncertain(c["geom"], c["angles"], c["ranges"], distinct).any(), name


def test_cell_picking_cases_have_the_shapes_their_tests_name():
    e = PC.eligibility_case()
    assert sorted(set(e["K"].tolist())) == list(range(9))
    keys = [R.key(s, k) for s, k in zip(e["S"], e["K"])]
    assert e["K"][int(np.argmax(keys))] == 4             # the greatest key: ineligible from min_known = 5 on
    for thr, need in PC.ELIGIBILITY_THRESHOLDS:
        assert R.min_known(8, thr) == need == api.host_min_known(8, thr)
    for first in PC.TIE_FIRST:
        c = PC.tie_case(first)
        holders = np.nonzero(c["S"] == c["S"].max())[0]
        assert holders[0] == first and set(c["S"].tolist()) == {20000, 60000}
        if first < PC.TIE_N - 1:
            assert len(set((holders // 64).tolist())) > 2 and len(set((holders // 1024).tolist())) > 1
        else:
            assert holders.size == 1
    c = PC.zero_runs_case("runs")
    w, _, info = R.update_fast(c["S"].tolist(), c["K"].tolist(), 1, PC.ZERO_TEMPERATURE)
    assert np.nonzero(w)[0].tolist() == c["weighted"].tolist() and len(set(w)) == 3
    assert not any(w[64:128]) and not any(w[1024:2048]) and w[63] and w[128] and w[1023] and w[2048]
    c = PC.tile_shape_case(1023)
    w, _, info = R.update_fast(c["S"].tolist(), c["K"].tolist(), 1, 0.3)
    assert sum(w[:1023]) > 1 << 32                       # the prefix sums pass 2^32 inside the first tile


def test_forced_poses_are_marked_and_few_others():
    c = PC.many_fixes_case()
    marked = R.margin_uncertain(c["geom"], c["angles"], c["ranges"], c["poses"])
    assert marked[list(c["forced"])].all() and marked.sum() <= 23 + 3
    run = [i for i in c["forced"] if 7 <= i <= 13]
    assert len(run) == 7 and {0, 299, 40, 41} <= set(c["forced"])
    grids, sets = PC.three_sets_case()
    assert [s["angles"].size for s in sets] == [65, 3, 1100, 65, 65, 3]
    assert [s["poses"].shape[0] for s in sets] == [70, 0, 9, 0, 130, 5]
    assert sets[0]["angles"] is sets[4]["angles"] and {s["map"] for s in sets} == {0, 1}
    for s in sets:
        if s["poses"].shape[0]:
            marked = R.margin_uncertain(s["geom"], s["angles"], s["ranges"], s["poses"])
            assert marked[list(s["forced"])].all() and len(s["forced"]) >= 2
            assert marked.sum() <= len(s["forced"]) + 1
    c = PC.two_batches_case()
    assert c["ranges"][0] == 0.0 and c["ranges"].min() >= 0.0 and c["ranges"].max() <= 1.0
    assert R.margin_uncertain(c["geom"], c["angles"], c["ranges"], c["poses"]).all()
    assert 129 * 2 * 65536 * 4 > 64 << 20 >= 128 * 2 * 65536 * 4
    rows, cols = c["grid"].shape
    assert np.abs(c["poses"][:, 0]).max() + 1.0 < 2.0 and np.abs(c["poses"][:, 1]).max() + 1.0 < 1.5


def test_generic_cases_stay_on_the_device_path():
    """At most 1 % of each generic case's poses inside the certificate's margin: a condition on the seeds."""
    for name, c in PC.frame_cases().items():
        marked = R.margin_uncertain(c["geom"], c["angles"], c["ranges"], c["poses"])
        assert marked.sum() <= c["poses"].shape[0] // 100, (name, int(marked.sum()))
        S, K = R.score_poses(c["grid"], c["geom"], c["angles"], c["ranges"], c["poses"][:40])
        assert K.max() > 0, name                         # the poses are on the map
    assert abs(np.abs(PC.frame_cases()["angles_x40_65"]["angles"]).max() - 125.0) < 1.0
    for gp in PC.LAYOUTS:
        grids, sets = PC.layout_case(gp)
        marked = sum(int(R.margin_uncertain(s["geom"], s["angles"], s["ranges"], s["poses"]).sum())
                     for s in sets if s["poses"].shape[0])
        assert marked <= sum(PC.LAYOUTS[gp]) // 100, (gp, marked)
    c = PC.accumulator_case()
    assert not R.margin_uncertain(c["geom"], c["angles"], c["ranges"], c["poses7"]).any()
    c = R.sweep_case(5, 33001)                           # the large call of the sequence test
    assert R.margin_uncertain(c["geom"], c["angles"], c["ranges"], c["poses"]).sum() <= 330


def test_accumulator_case_is_at_the_limit():
    c = PC.accumulator_case()
    S, K = R.score_poses(c["grid"], c["geom"], c["angles"], c["ranges"], c["poses"])
    assert S.tolist() == [PC.FULL_S] * 6 and K.tolist() == [PC.FULL_K] * 6 and PC.FULL_S == 0xFFFF0000
    rec = api.host_score_poses(c["grid_low"], c["geom"], c["angles"], c["ranges"], c["poses7"])
    S, K = R.score_poses(c["grid_low"], c["geom"], c["angles"], c["ranges"], c["poses7"])
    assert np.array_equal(R.records_sk(rec)[0], S) and np.array_equal(R.records_sk(rec)[1], K)
    assert S[:6].tolist() == [PC.FULL_S] * 6 and K.tolist() == [PC.FULL_K] * 7      # the six never reach the cell
    assert S[6] < PC.FULL_S and (PC.FULL_S - S[6]) % 65534 == 0
    assert R.key(PC.FULL_S, PC.FULL_K) < 1 << 42
    c2 = dict(S=S, K=K, n_points=65536)
    w, a, info = _assert_host_is_fast(c2, PC.ACC_TEMPERATURE, 0.5, 9, 12345)
    assert info["best_index"] == 0 and info["support"] == 7 and w[6] != w[0]
    score, rate = api.host_score_from_sums(int(S[6]), int(K[6]), 65536)
    assert np.isfinite(score) and score <= 1.0 and rate == 1.0
    assert api.host_score_from_sums(PC.FULL_S, PC.FULL_K, 65536)[0] <= 1.0


def test_update_fast_is_the_definition():
    rng = np.random.RandomState(5)
    K = rng.randint(100, 361, 500)
    S = K * rng.randint(20000, 60000, 500)
    K6 = np.random.RandomState(6).randint(0, 361, 211)
    S6 = K6 * np.random.RandomState(7).randint(1000, 65000, 211)
    cases = [([5000] * 37, [10] * 37, 360, 0.05, 0.0, 37, 0),
             ([100, 90000, 300, 7], [2, 200, 3, 1], 360, 0.02, 0.5, 9, 12345),
             ([100, 90000, 300, 7], [2, 200, 3, 1], 360, 0.02, 0.9, 9, 12345),
             (S.tolist(), K.tolist(), 360, 2e-4, 0.1, 500, 99),
             ([10, 20], [1, 1], 4, 0.05, 0.0, 0, 7),
             ([], [], 360, 0.05, 0.0, 3, 0)]
    for n_out in (1, 7, 211, 844):
        for offset in (0, (1 << 64) - 1, 0x123456789ABCDEF):
            cases.append((S6.tolist(), K6.tolist(), 360, 0.03, 0.2, n_out, offset))
    e = PC.eligibility_case()
    for thr, _ in PC.ELIGIBILITY_THRESHOLDS:
        cases.append((e["S"].tolist(), e["K"].tolist(), 8, 0.05, thr, 45, 11))
    t = PC.tie_case(64)
    cases.append((t["S"][:300].tolist(), t["K"][:300].tolist(), 1, 0.3, 0.0, 300, 5))
    z = PC.zero_runs_case("runs")
    cases.append((z["S"][:200].tolist(), z["K"][:200].tolist(), 1, PC.ZERO_TEMPERATURE, 0.0, 50, (1 << 64) - 1))
    for args in cases:
        assert R.update_fast(*args) == R.update(*args), args[2:]


def test_host_update_equals_update_fast_on_every_update_case():
    for n in PC.TILE_SHAPES:
        c = PC.tile_shape_case(n)
        _assert_host_is_fast(c, 0.3, 0.0, n, 77 + n)
        _assert_host_is_fast(c, 0.02, 0.0, 2 * n + 1, (1 << 64) - 1)
    for first in PC.TIE_FIRST:
        w, a, info = _assert_host_is_fast(PC.tie_case(first), 0.3, 0.0, PC.TIE_N, 5)
        assert info["best_index"] == first
    for layout in PC.ZERO_LAYOUTS:
        c = PC.zero_runs_case(layout)
        for n_out in (1, 7, 4 * PC.ZERO_N):
            for offset in (0, (1 << 64) - 1, 0x123456789ABCDEF):
                w, a, info = _assert_host_is_fast(c, PC.ZERO_TEMPERATURE, 0.0, n_out, offset)
                assert info["support"] == c["weighted"].size and set(a) <= set(c["weighted"].tolist())
    e = PC.eligibility_case()
    for thr, need in PC.ELIGIBILITY_THRESHOLDS:
        w, a, info = _assert_host_is_fast(e, 0.05, thr, 45, 11)
        assert info["found"] == (need <= 8)
        if info["found"]:
            assert e["K"][info["best_index"]] >= need and all(e["K"][i] >= need for i in a)
    n = PC.MAX_POSES
    c = PC.limit_case(False)
    for offset in ((1 << 64) - 1, 0):
        w, a, info = _assert_host_is_fast(c, 0.05, 0.0, n, offset)
        assert set(w) == {1 << 24} and info["m0"] == 1 << 42 and info["support"] == n and info["best_index"] == 0
        assert a == list(range(n))
    w, a, info = _assert_host_is_fast(PC.limit_case(True), 0.05, 0.0, n, 3)
    assert info["best_index"] == n - 1


def test_host_entry_limits():
    grid = R.make_map(1)
    poses = R.make_poses(1, 3)
    a, r = R.make_scan(1, 65537)
    assert _host_score_rc(grid, R.GEOM, a, r, poses, n_points=65536) == 0
    assert _host_score_rc(grid, R.GEOM, a, r, poses, n_points=65537) == L.CSM_EINVAL
    a, r = R.make_scan(1, 8)
    r[2], r[5] = 0.0, -0.7                                # a zero and a negative range are ranges like any other
    assert _host_score_rc(grid, R.GEOM, a, r, poses) == 0
    rec = api.host_score_poses(grid, R.GEOM, a, r, poses)
    S, K = R.score_poses(grid, R.GEOM, a, r, poses)
    assert np.array_equal(R.records_sk(rec)[0], S) and np.array_equal(R.records_sk(rec)[1], K)
