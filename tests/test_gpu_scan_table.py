"""The scans of a call are shared by their arrays AND their length: two entries that feed the same angle and
range arrays at different lengths are different scans. Each consumer that stages the distinct scans of a call
once (correlative_match_batch, construct_maps_from_scans, ray_check_batch, score_pose_sets) gets one call of
three entries on one small map -- scan A, A again through the same arrays, and the first n - 1 beams of A
through the same two base pointers -- and must return exactly what three separate calls on private copies of
the arrays return. Everything compared is an integer, a record of integers or a double both paths compute by
the same instructions, so the comparison is ==."""
import ctypes as C
import math

import numpy as np
import pytest

import map_batch_cases as M
import pose_set_reference as P
import ray_check_reference as R
from csm_hip import api, synth

pytestmark = pytest.mark.gpu

BASE = 9700                          # 9700 .. 9719: this file's map ids
CSM = (1.0, 1.0, math.radians(10), 4, 0.0, 0.0)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _entries(angles, ranges):
    """(angles, ranges) of the three entries: A, A again, the first n - 1 beams of A. The prefix views start at
    the arrays' own addresses, and the binding hands a contiguous float64 array over where it lies."""
    a, r = _f64(angles), _f64(ranges)
    n = a.size
    assert n > 2 and r.size == n
    out = [(a, r), (a, r), (a[:n - 1], r[:n - 1])]
    for x, y in out:
        assert api._f64(x).ctypes.data == a.ctypes.data and api._f64(y).ctypes.data == r.ctypes.data
    assert api._f64(out[2][0]).size == n - 1
    return out


def _private(entries):
    return [(np.copy(a), np.copy(r)) for a, r in entries]


def _scan_ptrs(prepared):
    return [(C.cast(q.scan.angles, C.c_void_p).value, C.cast(q.scan.ranges, C.c_void_p).value, q.scan.n_points)
            for q in prepared.arr]


def test_match_batch(gpu_ctx):
    c = synth.csm_case(1200, n_beams=64)
    gpu_ctx.upload_grid(BASE, c["grid"])
    try:
        def queries(entries):
            return [dict(map_id=BASE, geom=c["geom"], angles=a, ranges=r, rel_pose=c["rel_pose"],
                         init_pose=c["init_pose"]) for a, r in entries]

        def records(outs):
            return [(o["pose_found"], o["raw"], o["estimated_pose"], o["win_x"], o["win_y"], o["win_theta"])
                    for o in outs]

        entries = _entries(c["angles"], c["ranges"])
        prepared = gpu_ctx.prepare_queries(queries(entries))
        ptrs = _scan_ptrs(prepared)
        assert len({p[:2] for p in ptrs}) == 1 and [p[2] for p in ptrs] == [64, 64, 63]
        together = records(gpu_ctx.correlative_match_batch(prepared, *CSM))
        apart = [records(gpu_ctx.correlative_match_batch(queries([e]), *CSM))[0] for e in _private(entries)]
        assert together == apart
        assert together[0] == together[1] and together[0][1]["found"] == 1
    finally:
        gpu_ctx.release_grid(BASE)


def test_construct_maps_from_scans(gpu_ctx):
    (_, case), = M.build(["one_scan"])
    nd = case["nodes"][0]

    def jobs(entries, first_id):
        return [dict(map_id=first_id + j, shape=case["shape"], map_pose=case["map_pose"],
                     nodes=[dict(nd, angles=a, ranges=r)]) for j, (a, r) in enumerate(entries)]

    def strip(info):
        return {k: v for k, v in info.items() if not k.endswith("_us")}

    entries = _entries(nd["angles"], nd["ranges"])
    ids = list(range(BASE + 1, BASE + 7))
    try:
        together, binfo = gpu_ctx.construct_maps_from_scans(jobs(entries, ids[0]))
        apart = [gpu_ctx.construct_maps_from_scans(jobs([e], ids[3 + j]))[0][0]
                 for j, e in enumerate(_private(entries))]
        # the scan of the first two jobs went up once, the prefix on its own
        assert binfo["scan_bytes_uploaded"] == 16 * (2 * entries[0][0].size - 1)
        for j in range(3):
            assert together[j][2] == 0 and apart[j][2] == 0
            assert together[j][0] == apart[j][0]
            assert strip(together[j][1]) == strip(apart[j][1])
            assert np.array_equal(gpu_ctx.download_level(ids[j], 0), gpu_ctx.download_level(ids[3 + j], 0))
    finally:
        for i in ids:
            if gpu_ctx.has_grid(i):
                gpu_ctx.release_grid(i)


def test_ray_check_batch(gpu_ctx):
    c = next(k for k in R.named_cases() if k["name"] == "sensor_outside_low")
    gpu_ctx.upload_grid(BASE + 10, c["grid"])
    try:
        def queries(entries):
            return [dict(map_id=BASE + 10, geom=c["geom"], angles=a, ranges=r, rel_pose=c["rel_pose"],
                         init_pose=c["pose"]) for a, r in entries]

        entries = _entries(c["angles"], c["ranges"])
        n = entries[0][0].size
        got, words = gpu_ctx.ray_check_batch(queries(entries), per_beam=True, **c["params"])
        for j, e in enumerate(_private(entries)):
            one, one_words = gpu_ctx.ray_check_batch(queries([e]), per_beam=True, **c["params"])
            assert got[j] == one[0]
            assert np.array_equal(words[j], one_words[0])
        assert [g["beams"] for g in got] == [n, n, n - 1]
        assert np.array_equal(words[2], words[0][:n - 1])
    finally:
        gpu_ctx.release_grid(BASE + 10)


def test_score_pose_sets(gpu_ctx):
    grid = P.make_map(3)
    angles, ranges = P.make_scan(3, 37)
    poses = P.make_poses(3, 50)
    gpu_ctx.upload_grid(BASE + 11, grid)
    try:
        def sets(entries):
            return [dict(map_id=BASE + 11, geom=P.GEOM, angles=a, ranges=r, poses=poses) for a, r in entries]

        entries = _entries(angles, ranges)
        together, _ = gpu_ctx.score_pose_sets(sets(entries))
        for j, e in enumerate(_private(entries)):
            one, _ = gpu_ctx.score_pose_sets(sets([e]))
            assert np.array_equal(together[j], one[0])
        assert np.array_equal(together[0], together[1])
        assert not np.array_equal(together[0], together[2])
    finally:
        gpu_ctx.release_grid(BASE + 11)
