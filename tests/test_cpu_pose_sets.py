"""CPU suite of the pose sets: the host restatements inside libcsm_hip.so (csm_host_score_poses,
csm_host_score_from_sums, csm_host_pose_set_update) against the literal Python of tests/pose_set_reference.py
and the oracle's ScorePixelAccurate, their refusals, and the seeds of the GPU cases (the certificate's margin
in numpy must leave at most 1 % of a generic case's poses to the host)."""
import ctypes as C

import numpy as np
import pytest

import pose_set_reference as R
from csm_hip import _lib as L
from csm_hip import api


def _assert_update(rec_s, rec_k, n_points, temperature, threshold, n_out, offset):
    rec = np.zeros(len(rec_s), api.POSE_RECORD)
    rec["sum_values"], rec["known"] = rec_s, rec_k
    weights, ancestors, info = api.host_pose_set_update(rec, n_points, temperature, threshold, n_out, offset)
    want_w, want_a, want_info = R.update(rec_s, rec_k, n_points, temperature, threshold, n_out, offset)
    assert weights.tolist() == want_w
    assert ancestors.tolist() == want_a
    assert info == want_info
    return weights, ancestors, info


@pytest.mark.parametrize("seed, n_points, n_poses", [(1, 1, 5), (2, 63, 40), (3, 360, 60), (4, 1080, 12)])
def test_host_score_poses_equals_the_restatement(oracle, seed, n_points, n_poses):
    grid = R.make_map(seed)
    angles, ranges = R.make_scan(seed, n_points, 0.2, 2.5)           # some beams leave the map
    poses = R.make_poses(seed, n_poses, 1.5, 1.1)
    rec = api.host_score_poses(grid, R.GEOM, angles, ranges, poses)
    S, K = R.score_poses(grid, R.GEOM, angles, ranges, poses)
    got_s, got_k = R.records_sk(rec)
    assert np.array_equal(got_s, S) and np.array_equal(got_k, K)
    assert not rec["flags"].any() and not rec["reserved"].any()
    assert K.max() > 0 and (n_points == 1 or K.min() < n_points)
    for p in range(n_poses):
        want, known = oracle.score_at(grid, R.GEOM, angles, ranges, poses[p])
        score, rate = api.host_score_from_sums(S[p], K[p], n_points)
        assert known == K[p]
        assert abs(score - want) <= 1e-12, (p, score, want)
        assert rate == K[p] / n_points


def test_score_from_sums_is_the_fixed_expression():
    c = 0.998 / (65534.0 * 499.0)
    for s, k, n in ((0, 0, 1), (65535, 1, 1), (12345678, 300, 360), (1080 * 65535, 1080, 1080)):
        assert api.host_score_from_sums(s, k, n) == ((float(32268 * k + 499 * s) * c) / float(n), float(k) / float(n))
    with pytest.raises(api.CsmError):
        api.host_score_from_sums(1, 1, 0)


def test_update_all_poses_tied():
    n = 37
    w, a, info = _assert_update([5000] * n, [10] * n, 360, 0.05, 0.0, n, 0)
    assert set(w.tolist()) == {1 << 24} and info["best_index"] == 0 and info["support"] == n
    assert a.tolist() == list(range(n))


def test_update_one_eligible_and_none_eligible():
    S, K = [100, 90000, 300, 7], [2, 200, 3, 1]
    w, a, info = _assert_update(S, K, 360, 0.02, 0.5, 9, 12345)        # needs K >= 181: pose 1 alone
    assert info["found"] == 1 and info["best_index"] == 1 and info["support"] == 1
    assert w.tolist() == [0, 1 << 24, 0, 0] and a.tolist() == [1] * 9
    w, a, info = _assert_update(S, K, 360, 0.02, 0.9, 9, 12345)        # needs K >= 325: none
    assert info == dict(m0=0, key_max=0, best_index=-1, support=0, bin_shift=info["bin_shift"], found=0)
    assert not w.any() and a.tolist() == [-1] * 9


def test_update_small_temperature_leaves_most_weights_zero():
    rng = np.random.RandomState(5)
    n, n_points = 500, 360
    K = rng.randint(100, 361, n)
    S = K * rng.randint(20000, 60000, n)
    w, a, info = _assert_update(S.tolist(), K.tolist(), n_points, 2e-4, 0.1, n, 99)
    assert 1 <= info["support"] < n // 4
    assert set(a.tolist()) <= set(np.nonzero(w)[0].tolist())


@pytest.mark.parametrize("n_out_of", [lambda n: 1, lambda n: 7, lambda n: n, lambda n: 4 * n])
def test_update_output_counts_and_offsets(n_out_of):
    rng = np.random.RandomState(6)
    n, n_points = 211, 360
    K = rng.randint(0, 361, n)
    S = K * rng.randint(1000, 65000, n)
    offsets = [0, (1 << 64) - 1] + [int(rng.randint(0, 1 << 62)) * 3 + 1 for _ in range(3)]
    for offset in offsets:
        w, a, info = _assert_update(S.tolist(), K.tolist(), n_points, 0.03, 0.2, n_out_of(n), offset)
        assert info["found"] == 1 and (np.diff(a) >= 0).all()


def test_update_of_no_pose_and_no_output():
    w, a, info = api.host_pose_set_update(np.zeros(0, api.POSE_RECORD), 360, 0.05, 0.0, 3, 0)
    assert w.size == 0 and a.tolist() == [-1, -1, -1] and info["found"] == 0
    _assert_update([10, 20], [1, 1], 4, 0.05, 0.0, 0, 7)


def _host_score_rc(grid, geom, angles, ranges, poses, n_points=None, n_poses=None):
    sc, keep = api._scan_struct(angles, ranges, (0.0, 0.0, 0.0))
    if n_points is not None:
        sc.n_points = n_points
    p = np.ascontiguousarray(poses, np.float64).reshape(-1, 3)
    out = np.zeros(max(p.shape[0], 1), api.POSE_RECORD)
    return L.load().csm_host_score_poses(api._ptr(grid), grid.shape[0], grid.shape[1], C.byref(L.Geometry(*geom)),
                                         C.byref(sc), api._ptr(p), p.shape[0] if n_poses is None else n_poses,
                                         api._ptr(out))


def test_host_score_poses_refusals():
    grid = R.make_map(1)
    a, r = R.make_scan(1, 8)
    poses = R.make_poses(1, 3)
    assert _host_score_rc(grid, R.GEOM, a, r, poses) == 0
    assert _host_score_rc(grid, R.GEOM, a, r, poses[:0]) == 0                       # no pose: valid
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(3):
            q = poses.copy()
            q[1, k] = bad
            assert _host_score_rc(grid, R.GEOM, a, r, q) == L.CSM_EINVAL
        a2, r2 = a.copy(), r.copy()
        a2[3] = bad
        r2[5] = bad
        assert _host_score_rc(grid, R.GEOM, a2, r, poses) == L.CSM_EINVAL
        assert _host_score_rc(grid, R.GEOM, a, r2, poses) == L.CSM_EINVAL
    assert _host_score_rc(grid, R.GEOM, a, r, poses, n_points=0) == L.CSM_EINVAL
    assert _host_score_rc(grid, R.GEOM, a, r, poses, n_poses=-1) == L.CSM_EINVAL
    far = poses.copy()
    far[2, 0] = R.GEOM[1] + 0.05 * 2.0 ** 30                                        # cell coordinate 2^30
    assert _host_score_rc(grid, R.GEOM, a, r, far) == L.CSM_EINVAL
    far[2, 0] = R.GEOM[1] + 0.05 * 2.0 ** 29
    assert _host_score_rc(grid, R.GEOM, a, r, far) == 0
    far[2] = (0.0, R.GEOM[2] - 0.05 * 2.0 ** 30, 0.0)
    assert _host_score_rc(grid, R.GEOM, a, r, far) == L.CSM_EINVAL


def test_host_update_refusals():
    rec = np.zeros(4, api.POSE_RECORD)
    for kw in (dict(n_out=-1), dict(n_out=(1 << 18) + 1), dict(temperature=0.0), dict(temperature=np.nan),
               dict(temperature=-1.0), dict(temperature=1e300), dict(known_rate_threshold=np.nan)):
        args = dict(temperature=0.05, known_rate_threshold=0.0, n_out=4, offset=0)
        args.update(kw)
        with pytest.raises(api.CsmError) as e:
            api.host_pose_set_update(rec, 360, **args)
        assert e.value.code == L.CSM_EINVAL, kw
    with pytest.raises(api.CsmError):
        api.host_pose_set_update(np.zeros((1 << 18) + 1, api.POSE_RECORD), 360, 0.05)
    w, a, info = api.host_pose_set_update(np.zeros(1 << 18, api.POSE_RECORD), 360, 0.05, 0.0, 1 << 18)
    assert info["found"] == 0                                                       # the limits themselves pass


def test_gpu_case_seeds_leave_the_device_path():
    """The seeds of the GPU sweep: by the margin formula alone at most 1 % of a case's poses are uncertified
    (so the device path is what those tests exercise), and the forced case has its pose on the edge."""
    for n_points in R.SWEEP_POINTS:
        for n_poses in R.SWEEP_POSES:
            c = R.sweep_case(n_points, n_poses)
            marked = R.margin_uncertain(c["geom"], c["angles"], c["ranges"], c["poses"])
            assert marked.sum() <= n_poses // 100, (n_points, n_poses, int(marked.sum()))
    e = R.edge_case()
    assert R.margin_uncertain(e["geom"], e["angles"], e["ranges"], e["poses"]).tolist() == [True, False]
