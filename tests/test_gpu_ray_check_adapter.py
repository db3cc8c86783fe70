"""GPU parity of the C++ adapters' free-space check (host/csm_adapters.hpp: RayCheckSettings, CheckRays,
DetectChecked on both loop detectors, DetectPeaksChecked on the correlative one), run from a small driver on
three queries. The second query's map holds a partition the scan never saw: its best pose still scores (the
end points land on walls) and must be dropped, because its rays run through the partition. Records must equal
Context.ray_check_batch at the same poses; the kept sets must equal the rule applied in Python."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import ray_check_reference as R
from csm_hip import _lib as Lb, api, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANGE = (1.0, 1.0, math.radians(10))
L, HEIGHT, K = 4, 3, 3
SCORE, KNOWN = 0.1, 0.1
# at the true poses (host restatement): 0 and 2 of 360 beams blocked, 146 of 360 through the partition; 114 to 138
# of 360 end points on occupied cells (the rest are beams at the scanner's maximum range)
RULE = dict(max_blocked_rate=0.1, min_walked=100, min_end_occupied_rate=0.1)
BASE = 8600                          # 8600 .. 8699: this file's ids on gpu_ctx (the driver has contexts of its own)

_CPP = r"""
#include <cstdio>
#include <vector>
#include "../my-lidar-graph-slam-v2_amd/host/csm_adapters.hpp"
using namespace CsmHip;
static FILE* o;
static void put(const CheckedLoopDetections& c)
{
    const int n = (int)c.mCandidates.size(), kept = (int)c.mResults.size();
    std::fwrite(&n, 4, 1, o);
    std::fwrite(&kept, 4, 1, o);
    for (int j = 0; j < n; ++j) {
        const int head[4] = { c.mQueryIndex[j], c.mPeakIndex[j], (int)c.mKept[j], 0 };
        const double pose[3] = { c.mCandidates[j].mRelativePose.mX, c.mCandidates[j].mRelativePose.mY,
                                 c.mCandidates[j].mRelativePose.mTheta };
        std::fwrite(head, 4, 4, o);
        std::fwrite(pose, 8, 3, o);
        std::fwrite(&c.mCandidateRecords[j], sizeof(csm_ray_check_result), 1, o);
    }
    for (int j = 0; j < kept; ++j) {
        const double pose[3] = { c.mResults[j].mRelativePose.mX, c.mResults[j].mRelativePose.mY,
                                 c.mResults[j].mRelativePose.mTheta };
        std::fwrite(pose, 8, 3, o);
        std::fwrite(&c.mRecords[j], sizeof(csm_ray_check_result), 1, o);
    }
}
int main(int argc, char** argv)
{
    /* input: rows cols n_queries n_beams; settings: range min max, occupied free (u32), tolerance, scale, min walked
     * (i32), rates[2]; per query: geom[3] rel[3] init[3], cells, angles, ranges */
    if (argc < 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    int hdr[4]; double rng[2]; unsigned thr[2]; int ints[3]; double rates[2];
    if (!f || std::fread(hdr, 4, 4, f) != 4 || std::fread(rng, 8, 2, f) != 2 || std::fread(thr, 4, 2, f) != 2 ||
        std::fread(ints, 4, 3, f) != 3 || std::fread(rates, 8, 2, f) != 2) return 2;
    const std::size_t nc = (std::size_t)hdr[0] * hdr[1], nb = (std::size_t)hdr[3];
    const int nq = hdr[2];
    std::vector<std::vector<std::uint16_t>> cells(nq, std::vector<std::uint16_t>(nc));
    std::vector<std::vector<double>> a(nq, std::vector<double>(nb)), r(nq, std::vector<double>(nb));
    LoopDetectionQueryVector queries(nq);
    std::vector<RobotPose2D<double>> inits(nq);
    for (int i = 0; i < nq; ++i) {
        double g[3], rel[3], init[3];
        if (std::fread(g, 8, 3, f) != 3 || std::fread(rel, 8, 3, f) != 3 || std::fread(init, 8, 3, f) != 3 ||
            std::fread(cells[i].data(), 2, nc, f) != nc || std::fread(a[i].data(), 8, nb, f) != nb ||
            std::fread(r[i].data(), 8, nb, f) != nb) return 2;
        LoopDetectionQuery& q = queries[i];
        q.mReferenceLocalMap.mValues = cells[i].data();
        q.mReferenceLocalMap.mRows = hdr[0]; q.mReferenceLocalMap.mCols = hdr[1];
        q.mReferenceLocalMap.mResolution = g[0]; q.mReferenceLocalMap.mPosOffsetX = g[1];
        q.mReferenceLocalMap.mPosOffsetY = g[2];
        q.mReferenceLocalMap.mId = 40 + i;
        q.mQueryScanData.mAngles = a[i].data(); q.mQueryScanData.mRanges = r[i].data();
        q.mQueryScanData.mNumOfScans = nb;
        q.mQueryScanData.mRelativeSensorPose = { rel[0], rel[1], rel[2] };
        q.mQueryScanNodeGlobalPose = { init[0], init[1], init[2] };
        q.mReferenceLocalMapNodeGlobalPose = { 0.0, 0.0, 0.0 };
        q.mQueryScanNodeId = 100 + i;
        inits[i] = { init[0], init[1], init[2] };
    }
    std::fclose(f);
    o = std::fopen(argv[2], "wb");
    if (!o) return 2;

    RayCheckSettings s = RayCheckSettings::Create(rng[0], rng[1]);
    const double size = (double)sizeof(csm_ray_check_result);
    std::fwrite(&size, 8, 1, o);
    std::fwrite(&s.mParams.occupied_min, 4, 1, o);      /* the defaults: P >= 0.65 / P <= 0.35 */
    std::fwrite(&s.mParams.free_max, 4, 1, o);
    s.mParams.occupied_min = thr[0]; s.mParams.free_max = thr[1];
    s.mParams.end_tolerance = ints[0]; s.mParams.subpixel_scale = ints[1];
    s.mMinWalked = ints[2]; s.mMaxBlockedRate = rates[0]; s.mMinEndOccupiedRate = rates[1];

    auto corr = LoopDetectorCorrelativeHIP::Create("corr", LOW_RES, 1.0, 1.0, RANGE_T, SCORE_T, KNOWN_T);
    auto bnb = LoopDetectorBranchBoundHIP::Create("bnb", HEIGHT_MAX, 1.0, 1.0, RANGE_T, SCORE_T, KNOWN_T);
    if (!corr || !bnb) return 3;
    for (int pass = 0; pass < 2; ++pass) {
        const std::vector<csm_ray_check_result> rec = pass ? bnb->CheckRays(queries, inits, s)
                                                           : corr->CheckRays(queries, inits, s);
        std::fwrite(rec.data(), sizeof(csm_ray_check_result), rec.size(), o);
    }
    const std::size_t plain = corr->Detect(queries).size();
    put(corr->DetectChecked(queries, s));
    put(bnb->DetectChecked(queries, s));
    put(corr->DetectPeaksChecked(queries, PEAKS, 2, 2, 1, s));
    const double same = corr->Detect(queries).size() == plain ? (double)plain : -1.0;
    std::fwrite(&same, 8, 1, o);
    std::fclose(o);
    return 0;
}
"""


def _cases():
    a, c = synth.csm_case(0), synth.csm_case(2)
    b = dict(a)
    grid = a["grid"].copy()
    res, off_x, off_y = a["geom"]
    half_y = float(a["segs"][0][1])                          # the room's first wall: (-hx, -hy, hx, -hy)
    col = int((a["truth"][0] + 1.5 - off_x) / res)           # a partition 1.5 m from the sensor, wall to wall
    r0, r1 = int((half_y - off_y) / res), int((-half_y - off_y) / res)
    grid[min(r0, r1):max(r0, r1) + 1, col:col + 2] = 60000
    b["grid"] = grid
    return [a, b, c]


def _read(blob, at, n_rec_size):
    n, kept = np.frombuffer(blob, np.int32, 2, at[0])
    at[0] += 8
    cands = []
    for _ in range(n):
        head = np.frombuffer(blob, np.int32, 4, at[0])
        pose = np.frombuffer(blob, np.float64, 3, at[0] + 16).tolist()
        rec = Lb.RayCheckResult.from_buffer_copy(blob[at[0] + 40:at[0] + 40 + n_rec_size])
        at[0] += 40 + n_rec_size
        cands.append(dict(query=int(head[0]), peak=int(head[1]), kept=bool(head[2]), pose=pose,
                          record=R.strip(api.ray_check_to_dict(rec))))
    results = []
    for _ in range(kept):
        pose = np.frombuffer(blob, np.float64, 3, at[0]).tolist()
        rec = Lb.RayCheckResult.from_buffer_copy(blob[at[0] + 24:at[0] + 24 + n_rec_size])
        at[0] += 24 + n_rec_size
        results.append((pose, R.strip(api.ray_check_to_dict(rec))))
    return cands, results


def test_cpp_adapters_check_rays_and_drop_the_pose_through_a_wall(gpu_ctx, tmp_path):
    text = (_CPP.replace("../my-lidar-graph-slam-v2_amd", os.path.join(ROOT, "my-lidar-graph-slam-v2_amd"))
            .replace("LOW_RES", str(L)).replace("HEIGHT_MAX", str(HEIGHT)).replace("PEAKS", str(K))
            .replace("RANGE_T", repr(RANGE[2])).replace("SCORE_T", repr(SCORE)).replace("KNOWN_T", repr(KNOWN)))
    src, exe = tmp_path / "rays.cpp", tmp_path / "rays"
    src.write_text(text)
    csrc = os.path.join(ROOT, "my-lidar-graph-slam-v2_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L" + csrc, "-lcsm_hip", "-Wl,-rpath," + csrc])
    cases = _cases()
    prm = R.params(usable_range_max=6.0)
    shape = cases[0]["grid"].shape
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.array([shape[0], shape[1], len(cases), cases[0]["angles"].size], np.int32).tobytes())
        f.write(np.array([prm["usable_range_min"], prm["usable_range_max"]], np.float64).tobytes())
        f.write(np.array([prm["occupied_min"], prm["free_max"]], np.uint32).tobytes())
        f.write(np.array([prm["end_tolerance"], prm["subpixel_scale"], RULE["min_walked"]], np.int32).tobytes())
        f.write(np.array([RULE["max_blocked_rate"], RULE["min_end_occupied_rate"]], np.float64).tobytes())
        for c in cases:
            assert c["grid"].shape == shape and c["angles"].size == cases[0]["angles"].size
            f.write(np.array(c["geom"], np.float64).tobytes())
            f.write(np.array(c["rel_pose"], np.float64).tobytes())
            f.write(np.array(c["init_pose"], np.float64).tobytes())
            f.write(np.ascontiguousarray(c["grid"], np.uint16).tobytes())
            f.write(np.asarray(c["angles"], np.float64).tobytes())
            f.write(np.asarray(c["ranges"], np.float64).tobytes())
    subprocess.check_call([str(exe), str(inp), str(outp)], timeout=120)
    blob = outp.read_bytes()
    size = C.sizeof(Lb.RayCheckResult)
    assert np.frombuffer(blob, np.float64, 1, 0)[0] == float(size)
    assert tuple(np.frombuffer(blob, np.uint32, 2, 8)) == api.host_ray_check_values(0.65, 0.35)
    at = [16]

    queries = [dict(map_id=BASE + i, geom=c["geom"], angles=c["angles"], ranges=c["ranges"], rel_pose=c["rel_pose"],
                    init_pose=c["init_pose"]) for i, c in enumerate(cases)]
    try:
        for q, c in zip(queries, cases):
            gpu_ctx.upload_grid(q["map_id"], c["grid"])

        def records_at(idx, poses):
            got = gpu_ctx.ray_check_batch([queries[i] for i in idx], poses=poses, **prm)
            return [R.strip(g) for g in got]

        # CheckRays at the initial poses, on both detectors
        want = records_at(range(len(cases)), [c["init_pose"] for c in cases])
        for _ in range(2):
            for w in want:
                rec = Lb.RayCheckResult.from_buffer_copy(blob[at[0]:at[0] + size])
                at[0] += size
                assert R.strip(api.ray_check_to_dict(rec)) == w

        def compare(found, first_only):
            """found: (query, peak, pose) of every candidate the detector had, in order."""
            cands, results = _read(blob, at, size)
            assert [(c["query"], c["peak"], c["pose"]) for c in cands] == [(q, p, list(pose)) for q, p, pose in found]
            want = records_at([q for q, _, _ in found], [pose for _, _, pose in found])
            assert [c["record"] for c in cands] == want
            passes = [R.check_passes(w, **RULE) for w in want]
            kept, taken = [], set()
            for (q, _, _), ok in zip(found, passes):
                kept.append(ok and not (first_only and q in taken))
                if kept[-1]:
                    taken.add(q)
            assert [c["kept"] for c in cands] == kept
            assert results == [(c["pose"], c["record"]) for c in cands if c["kept"]]
            return cands

        corr = gpu_ctx.correlative_match_batch(queries, *RANGE, L, SCORE, KNOWN)
        assert all(s["pose_found"] for s in corr)
        cands = compare([(i, 0, s["estimated_pose"]) for i, s in enumerate(corr) if s["pose_found"]], False)
        assert [c["kept"] for c in cands] == [True, False, True]      # the pose through the partition is dropped
        assert cands[1]["record"]["blocked"] > 0.1 * cands[1]["record"]["walked"]
        bnb = gpu_ctx.bnb_match_batch(queries, *RANGE, HEIGHT, SCORE, KNOWN)
        cands = compare([(i, 0, s["estimated_pose"]) for i, s in enumerate(bnb) if s["pose_found"]], False)
        assert [c["kept"] for c in cands if c["query"] == 1] == [False]
        peaks = gpu_ctx.correlative_peaks_batch(queries, *RANGE, L, K, excl=(2, 2, 1), score_threshold=SCORE,
                                                known_rate_threshold=KNOWN)
        assert max(len(p) for p in peaks) > 1
        cands = compare([(i, j, s["estimated_pose"]) for i, p in enumerate(peaks) for j, s in enumerate(p)], True)
        assert not any(c["kept"] for c in cands if c["query"] == 1)
        assert sorted(c["query"] for c in cands if c["kept"]) == [0, 2]
        assert np.frombuffer(blob, np.float64, 1, at[0])[0] == float(len(corr))     # Detect() itself is unchanged
        assert at[0] + 8 == len(blob)
    finally:
        for q in queries:
            if gpu_ctx.has_grid(q["map_id"]):
                gpu_ctx.release_grid(q["map_id"])
