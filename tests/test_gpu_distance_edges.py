"""GPU parity of the distance fields at the numbers their index arithmetic branches on: pad columns over an id
that held a larger map, the clamp at R^2, keep_unknown, the first-known counters, and the C++ adapter's option
(host/csm_adapters.hpp: ScanMatcherCorrelativeHIP::UseDistanceField), run from a small driver. Every claim
about a case is proved in tests/test_cpu_distance_reference.py. Bar: equality of bytes and double bits."""
import math
import os
import subprocess

import numpy as np
import pytest

import distance_reference as DR
from csm_hip import api, synth
from test_gpu_likelihood import _strip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC, DST, BIG = 8600, 8601, 8602            # 8600 .. 8699: this file's ids on gpu_ctx
RANGE = (1.0, 1.0, math.radians(10))
L = 4


def _release(ctx, *ids):
    for m in ids:
        if ctx.has_grid(m):
            ctx.release_grid(m)


@pytest.mark.parametrize("name", ["pad70", "pad130"])
def test_pad_columns_over_an_id_that_held_a_larger_map(gpu_ctx, name):
    """pitch > cols: pad cells read as no obstacle and are written 0. The destination held a larger map full of
    obstacles, and so did the source's id: whatever lay in either buffer before must not show."""
    g, t, want = DR.field_expected(name, 16, "ramp", 32768, False)
    full = np.full((150, 150), 60000, np.uint16)
    try:
        gpu_ctx.upload_grid(DST, full)
        gpu_ctx.upload_grid(SRC, full)
        gpu_ctx.upload_grid(SRC, g)
        gpu_ctx.build_distance_map(SRC, DST, radius=16, table=t)
        assert np.array_equal(gpu_ctx.download_level(DST, 0), want)
        # what is derived from the pitched rows equals what is derived from an upload (whose pad cells are 0)
        gpu_ctx.upload_grid(BIG, want)
        for m in (DST, BIG):
            gpu_ctx.build_pyramid(m, [1, 4])
        assert np.array_equal(gpu_ctx.download_level(DST, 1), gpu_ctx.download_level(BIG, 1))
        d2, nearest = gpu_ctx.distance_transform(SRC)
        assert np.array_equal(d2, DR.expected(name)[1]) and np.array_equal(nearest, DR.expected(name)[2])
    finally:
        _release(gpu_ctx, SRC, DST, BIG)


@pytest.mark.parametrize("R", DR.CLAMP_RADII)
def test_the_clamp_takes_the_last_entry_from_the_radius_on(gpu_ctx, R):
    """The ramp differs at every index: a cell at d2 = R^2 and every cell beyond get T[R^2], the cell with the
    largest d2 below R^2 its own entry."""
    t = DR.table_of("ramp", R)
    try:
        for name in ("clamp2x300", "far200"):
            g, d2, _ = DR.expected(name)
            gpu_ctx.upload_grid(SRC, g)
            gpu_ctx.build_distance_map(SRC, DST, radius=R, table=t)
            got = gpu_ctx.download_level(DST, 0)
            assert (got[d2 >= R * R] == t[R * R]).all()
            below = d2 < R * R
            assert np.array_equal(got[below], t[d2[below]])
            if name == "clamp2x300":
                for v in (R * R, R * R + 1):
                    assert (d2 == v).any()
                assert int(got[d2 == d2[below].max()][0]) == int(t[d2[below].max()]) != int(t[R * R])
            else:
                assert int((d2 > 255 * 255).sum()) == 765 and (R < 255 or int((got == t[R * R]).sum()) >= 765)
    finally:
        _release(gpu_ctx, SRC, DST)


@pytest.mark.parametrize("keep_unknown", [False, True])
def test_keep_unknown_on_a_map_with_an_unknown_band(gpu_ctx, keep_unknown):
    g, t, want = DR.field_expected("low_known", 16, "gauss", 32768, keep_unknown)
    try:
        gpu_ctx.upload_grid(SRC, g)
        assert gpu_ctx.debug_grid_known(SRC) == (9, 11)
        gpu_ctx.build_distance_map(SRC, DST, radius=16, keep_unknown=keep_unknown, table=t)
        got = gpu_ctx.download_level(DST, 0)
        assert np.array_equal(got, want)
        assert ((got == 0) == (g == 0)).all() if keep_unknown else (got != 0).all()
        assert gpu_ctx.debug_grid_known(DST) == ((9, 11) if keep_unknown else (0, 0))
    finally:
        _release(gpu_ctx, SRC, DST)


def test_first_known_counters(gpu_ctx):
    g = DR.grid_of("low_known")
    d2 = DR.expected("low_known")[1]
    try:
        gpu_ctx.upload_grid(SRC, g)
        source = gpu_ctx.debug_grid_known(SRC)
        # T[R^2] > 0, every cell known
        gpu_ctx.build_distance_map(SRC, DST, radius=3, table=DR.table_of("gauss", 3))
        assert gpu_ctx.debug_grid_known(DST) == (0, 0)
        # T[R^2] = 0: the first row / column within R of an obstacle
        gpu_ctx.build_distance_map(SRC, DST, radius=3, table=DR.table_of("cut", 3))
        rr, cc = np.nonzero(d2 < 9)
        assert gpu_ctx.debug_grid_known(DST) == (int(rr.min()), int(cc.min())) != (0, 0)
        # keep_unknown: never below the source's
        for kind in ("gauss", "cut"):
            gpu_ctx.build_distance_map(SRC, DST, radius=3, keep_unknown=True, table=DR.table_of(kind, 3))
            known = gpu_ctx.debug_grid_known(DST)
            assert known[0] >= source[0] and known[1] >= source[1]
            assert known == DR.first_known(DR.distance_map(g, DR.table_of(kind, 3), 3, keep_unknown=True))
        # a table of zeros: no known cell
        gpu_ctx.build_distance_map(SRC, DST, radius=3, table=DR.table_of("zeros", 3))
        assert gpu_ctx.debug_grid_known(DST) == g.shape
        assert not gpu_ctx.download_level(DST, 0).any()
    finally:
        _release(gpu_ctx, SRC, DST)


def test_a_rebuilt_field_is_a_new_map_to_the_search(gpu_ctx):
    """The state contract on an id that exists: a field that was matched on is rebuilt from other cells at
    another radius; the next match equals a fresh upload's (the derived copies were dropped, not reused)."""
    a, b = synth.csm_case(0), synth.csm_case(2)
    scan = (a["geom"], a["angles"], a["ranges"], a["rel_pose"], a["init_pose"])
    match = lambda m: _strip(gpu_ctx.correlative_match(m, *scan, *RANGE, L))
    try:
        gpu_ctx.upload_grid(SRC, a["grid"])
        gpu_ctx.build_distance_map(SRC, DST, 0.25, a["geom"][0])
        first = [match(DST) for _ in range(5)]                  # until the launch chain replays as a graph
        assert first[1:] == first[:-1]
        gpu_ctx.upload_grid(SRC, b["grid"])
        gpu_ctx.build_distance_map(SRC, DST, 1.0, a["geom"][0], 100)
        want = api.host_distance_map(b["grid"], 1.0, a["geom"][0], 100)
        assert np.array_equal(gpu_ctx.download_level(DST, 0), want)
        gpu_ctx.upload_grid(BIG, want)
        fresh = match(BIG)
        assert [match(DST), match(DST)] == [fresh, fresh] and fresh != first[0]
    finally:
        _release(gpu_ctx, SRC, DST, BIG)


_CPP = r"""
#include <cstdio>
#include <vector>
#include "../my-lidar-graph-slam-v2_amd/host/csm_adapters.hpp"
using namespace CsmHip;
static FILE* o;
static void put(double v) { std::fwrite(&v, 8, 1, o); }
static void put(const ScanMatchingSummary& s)
{
    const double v[19] = { s.mEstimatedPose.mX, s.mEstimatedPose.mY, s.mEstimatedPose.mTheta, s.mScoreValue,
                           (double)s.mFlags, s.mNormalizedCost,
                           s.mEstimatedCovariance[0], s.mEstimatedCovariance[1], s.mEstimatedCovariance[2],
                           s.mEstimatedCovariance[3], s.mEstimatedCovariance[4], s.mEstimatedCovariance[5],
                           s.mEstimatedCovariance[6], s.mEstimatedCovariance[7], s.mEstimatedCovariance[8],
                           s.mPoseFound ? 1.0 : 0.0, s.mBestSensorPose.mX, s.mBestSensorPose.mY,
                           s.mBestSensorPose.mTheta };
    std::fwrite(v, 8, 19, o);
}
static void put_cells(csm_ctx* ctx, std::uint64_t id, std::size_t n)
{
    std::vector<std::uint16_t> cells(n, 0xabcd);
    CSM_ASSERT_OK(ctx, csm_download_level(ctx, id, 0, cells.data()));
    std::fwrite(cells.data(), 2, n, o);
}
int main(int argc, char** argv)
{
    /* input: rows cols, res offx offy, n L, rel[3], init[3], range_theta, grid A, grid B, angles, ranges.
     * n * 2 bytes of cells is a multiple of 8 (checked by the test): the doubles stay aligned */
    if (argc < 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    int hdr[2]; double g[3]; int n[2]; double rel[3], init[3], rt;
    if (!f || std::fread(hdr, 4, 2, f) != 2 || std::fread(g, 8, 3, f) != 3 || std::fread(n, 4, 2, f) != 2 ||
        std::fread(rel, 8, 3, f) != 3 || std::fread(init, 8, 3, f) != 3 || std::fread(&rt, 8, 1, f) != 1) return 2;
    const std::size_t nc = (std::size_t)hdr[0] * hdr[1];
    std::vector<std::uint16_t> A(nc), B(nc);
    std::vector<double> a(n[0]), r(n[0]);
    if (std::fread(A.data(), 2, nc, f) != nc || std::fread(B.data(), 2, nc, f) != nc ||
        std::fread(a.data(), 8, n[0], f) != (size_t)n[0] || std::fread(r.data(), 8, n[0], f) != (size_t)n[0]) return 2;
    std::fclose(f);
    o = std::fopen(argv[2], "wb");
    if (!o) return 2;

    auto m = ScanMatcherCorrelativeHIP::Create("LocalSlam.ScanMatcherCorrelative", n[1], 1.0, 1.0, rt);
    if (!m) return 3;
    m->UseDeviceCostFunction(1e4);
    csm_ctx* ctx = m->Context();
    const std::uint64_t field = GridMapView::FieldId(7, GridMapView::kDistanceIdBit);
    put((double)(field == (7 | 1ull << 62)));
    ScanMatchingQuery q;
    q.mGridMap.mValues = A.data(); q.mGridMap.mRows = hdr[0]; q.mGridMap.mCols = hdr[1];
    q.mGridMap.mResolution = g[0]; q.mGridMap.mPosOffsetX = g[1]; q.mGridMap.mPosOffsetY = g[2];
    q.mGridMap.mId = 7;
    q.mScanData.mAngles = a.data(); q.mScanData.mRanges = r.data(); q.mScanData.mNumOfScans = (size_t)n[0];
    q.mScanData.mRelativeSensorPose = { rel[0], rel[1], rel[2] };
    q.mMapLocalInitialPose = { init[0], init[1], init[2] };

    put(m->OptimizePose(q));                                    /* 1: plain */
    put((double)csm_has_grid(ctx, field));
    m->UseDistanceField(0.5, 40);
    put(m->OptimizePose(q));                                    /* 2: on the field, built on first use */
    put((double)csm_has_grid(ctx, field));
    put_cells(ctx, field, nc);
    q.mGridMap.mValues = B.data();
    put(m->OptimizePose(q));                                    /* 3: other cells, same revision: the cache */
    q.mGridMap.mRevision = 1;
    put(m->OptimizePose(q));                                    /* 4: revised: map and field rebuilt */
    put_cells(ctx, field, nc);
    ScanMatchingQuery t = q;
    t.mGridMap.mValues = A.data();
    t.mGridMap.mId = GridMapView::kInvalidId;
    t.mGridMap.mRevision = 0;
    put(m->OptimizePose(t));                                    /* 5: a throw-away map */
    put((double)csm_has_grid(ctx, GridMapView::kReservedIds));
    put((double)csm_has_grid(ctx, GridMapView::FieldId(GridMapView::kReservedIds, GridMapView::kDistanceIdBit)));
    put((double)csm_has_grid(ctx, 7));
    put((double)csm_has_grid(ctx, field));
    m->UseDistanceField(0.25);                                  /* 6: the default radius, revision unchanged */
    put(m->OptimizePose(q));
    put_cells(ctx, field, nc);
    m->UseDistanceField(0.0);
    put(m->OptimizePose(q));                                    /* 7: plain again, second grid */
    std::fclose(o);
    return 0;
}
"""


def _row(m, cost):
    return (list(m["estimated_pose"]) + [m["raw"]["score"], float(m["raw"]["flags"]), cost["normalized_cost"]]
            + cost["covariance"].reshape(-1).tolist() + [float(m["pose_found"])] + list(m["best_sensor_pose"]))


def _expected(ctx, case, cells, occupancy):
    """The row of a search on `cells` with cost and covariance from `occupancy` at the winner's sensor pose."""
    scan = (case["geom"], case["angles"], case["ranges"], case["rel_pose"], case["init_pose"])
    try:
        ctx.upload_grid(DST, cells)
        ctx.upload_grid(SRC, occupancy)
        m = ctx.correlative_match(DST, *scan, *RANGE, L)
        q = [dict(map_id=SRC, geom=case["geom"], angles=case["angles"], ranges=case["ranges"],
                  rel_pose=case["rel_pose"], init_pose=case["init_pose"])]
        cost = ctx.cost_covariance_batch(q, [m["best_sensor_pose"]], 1e4)[0]
    finally:
        _release(ctx, SRC, DST)
    return _row(m, cost)


def test_cpp_adapter_searches_the_distance_field_and_follows_the_revision(gpu_ctx, tmp_path):
    src = tmp_path / "field.cpp"
    src.write_text(_CPP.replace("../my-lidar-graph-slam-v2_amd", os.path.join(ROOT, "my-lidar-graph-slam-v2_amd")))
    exe = tmp_path / "field"
    csrc = os.path.join(ROOT, "my-lidar-graph-slam-v2_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + csrc, "-lcsm_hip", "-Wl,-rpath," + csrc])
    c = synth.csm_case(0)
    A = np.ascontiguousarray(c["grid"], np.uint16)
    B = np.ascontiguousarray(synth.csm_case(2)["grid"], np.uint16)
    assert A.shape == B.shape and (A != B).any() and A.size % 4 == 0
    res = c["geom"][0]
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.array(A.shape, np.int32).tobytes())
        f.write(np.array(c["geom"], np.float64).tobytes())
        f.write(np.array([len(c["angles"]), L], np.int32).tobytes())
        f.write(np.array(c["rel_pose"], np.float64).tobytes())
        f.write(np.array(c["init_pose"], np.float64).tobytes())
        f.write(np.array([RANGE[2]], np.float64).tobytes())
        f.write(A.tobytes())
        f.write(B.tobytes())
        f.write(np.asarray(c["angles"], np.float64).tobytes())
        f.write(np.asarray(c["ranges"], np.float64).tobytes())
    subprocess.check_call([str(exe), str(inp), str(outp)], timeout=120)
    blob = outp.read_bytes()
    at = [0]

    def doubles(n):
        v = np.frombuffer(blob, np.float64, n, at[0]).tolist()
        at[0] += 8 * n
        return v

    def cells():
        v = np.frombuffer(blob, np.uint16, A.size, at[0]).reshape(A.shape)
        at[0] += 2 * A.size
        return v

    # the references: the fields by the Python entry's host function, the rows on gpu_ctx
    field_a, field_b = api.host_distance_map(A, 0.5, res, 40), api.host_distance_map(B, 0.5, res, 40)
    field_b15 = api.host_distance_map(B, 0.25, res)
    assert DR.radius(0.25, res) == 15 and (field_b15 != field_b).any()
    plain_a, plain_b = _expected(gpu_ctx, c, A, A), _expected(gpu_ctx, c, B, B)
    on_a, on_b, on_b15 = (_expected(gpu_ctx, c, field_a, A), _expected(gpu_ctx, c, field_b, B),
                          _expected(gpu_ctx, c, field_b15, B))
    # what a wrong adapter would return instead must be another row
    assert on_a != plain_a and on_a != _expected(gpu_ctx, c, field_a, field_a)
    assert on_a != on_b and on_b != on_b15 and plain_a != plain_b

    assert doubles(1) == [1.0]                          # the field's id is 7 | 1 << 62
    assert doubles(19) == plain_a                       # 1
    assert doubles(1) == [0.0]                          # no field before the option
    assert doubles(19) == on_a                          # 2
    assert doubles(1) == [1.0]
    assert np.array_equal(cells(), field_a)             # the cells of the Python entry
    assert doubles(19) == on_a                          # 3: same revision, the resident map and field
    assert doubles(19) == on_b                          # 4
    assert np.array_equal(cells(), field_b)
    assert doubles(19) == on_a                          # 5
    assert doubles(4) == [0.0, 0.0, 1.0, 1.0]           # neither throw-away id is left; id 7 and its field are
    assert doubles(19) == on_b15                        # 6
    assert np.array_equal(cells(), field_b15)
    assert doubles(19) == plain_b                       # 7
    assert at[0] == len(blob)
