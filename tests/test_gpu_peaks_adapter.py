"""GPU parity of the C++ adapters' peak entries (host/csm_adapters.hpp): ScanMatcherCorrelativeHIP::
OptimizePosePeaks and LoopDetectorCorrelativeHIP::DetectPeaks, run from a small driver, against
tests/peaks_reference.py; OptimizePose / Detect beside them must give the first peak."""
import math
import os
import subprocess

import numpy as np
import pytest

import peaks_reference as PR
from csm_hip import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANGE = (1.0, 1.0, math.radians(10))
K_MAX, EXCL = 4, (3, 3, 2)
DETECTOR_THR = (0.3, 0.5)      # score, known rate: the detector's constructor wants both in (0, 1]

_CPP = r"""
#include <cstdio>
#include <vector>
#include "../my-lidar-graph-slam-v2_amd/host/csm_adapters.hpp"
using namespace CsmHip;
static void put(FILE* o, const double pose[3], double score, std::uint32_t flags)
{
    const double v[5] = { pose[0], pose[1], pose[2], score, (double)flags };
    std::fwrite(v, 8, 5, o);
}
int main(int argc, char** argv)
{
    /* input: rows cols res offx offy n L relx rely relt initx inity initt range_theta, grid, angles, ranges */
    if (argc < 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    int hdr[2]; double g[3]; int n[2]; double rel[3], init[3], rt;
    if (!f || std::fread(hdr, 4, 2, f) != 2 || std::fread(g, 8, 3, f) != 3 || std::fread(n, 4, 2, f) != 2 ||
        std::fread(rel, 8, 3, f) != 3 || std::fread(init, 8, 3, f) != 3 ||
        std::fread(&rt, 8, 1, f) != 1) return 2;
    std::vector<std::uint16_t> cells((size_t)hdr[0] * hdr[1]);
    std::vector<double> a(n[0]), r(n[0]);
    if (std::fread(cells.data(), 2, cells.size(), f) != cells.size() || std::fread(a.data(), 8, n[0], f) != (size_t)n[0] ||
        std::fread(r.data(), 8, n[0], f) != (size_t)n[0]) return 2;
    std::fclose(f);
    FILE* o = std::fopen(argv[2], "wb");

    auto m = ScanMatcherCorrelativeHIP::Create("LocalSlam.ScanMatcherCorrelative", n[1], 1.0, 1.0, rt);
    if (!m) return 3;
    ScanMatchingQuery q;
    q.mGridMap.mValues = cells.data(); q.mGridMap.mRows = hdr[0]; q.mGridMap.mCols = hdr[1];
    q.mGridMap.mResolution = g[0]; q.mGridMap.mPosOffsetX = g[1]; q.mGridMap.mPosOffsetY = g[2];
    q.mScanData.mAngles = a.data(); q.mScanData.mRanges = r.data(); q.mScanData.mNumOfScans = (size_t)n[0];
    q.mScanData.mRelativeSensorPose = { rel[0], rel[1], rel[2] };
    q.mMapLocalInitialPose = { init[0], init[1], init[2] };
    const std::vector<ScanMatchingSummary> peaks = m->OptimizePosePeaks(q, 4, 3, 3, 2);
    const ScanMatchingSummary one = m->OptimizePose(q);
    const double count = (double)peaks.size();
    std::fwrite(&count, 8, 1, o);
    for (const ScanMatchingSummary& s : peaks) {
        const double p[3] = { s.mEstimatedPose.mX, s.mEstimatedPose.mY, s.mEstimatedPose.mTheta };
        put(o, p, s.mScoreValue, s.mFlags);
    }
    const double p1[3] = { one.mEstimatedPose.mX, one.mEstimatedPose.mY, one.mEstimatedPose.mTheta };
    put(o, p1, one.mScoreValue, one.mFlags);

    auto d = LoopDetectorCorrelativeHIP::Create("LoopDetectorCorrelative", n[1], 1.0, 1.0, rt, 0.3, 0.5);
    if (!d) return 3;
    LoopDetectionQuery lq;
    lq.mReferenceLocalMap = q.mGridMap;
    lq.mReferenceLocalMap.mId = 5;
    lq.mQueryScanData = q.mScanData;
    lq.mReferenceLocalMapNodeGlobalPose = { 0.0, 0.0, 0.0 };     /* the map-local initial pose is then `init` */
    lq.mQueryScanNodeGlobalPose = { init[0], init[1], init[2] };
    lq.mQueryScanNodeId = 9;
    const LoopDetectionQueryVector queries { lq, lq };
    const std::vector<LoopDetectionResultVector> found = d->DetectPeaks(queries, 4, 3, 3, 2);
    const LoopDetectionResultVector first = d->Detect(queries);
    const double sizes[3] = { (double)found.size(), (double)found[1].size(), (double)first.size() };
    std::fwrite(sizes, 8, 3, o);
    for (const LoopDetectionResult& s : found[1]) {
        const double p[3] = { s.mRelativePose.mX, s.mRelativePose.mY, s.mRelativePose.mTheta };
        put(o, p, s.mScoreValue, s.mFlags);
    }
    const double p2[3] = { first[1].mRelativePose.mX, first[1].mRelativePose.mY, first[1].mRelativePose.mTheta };
    put(o, p2, first[1].mScoreValue, (std::uint32_t)first[1].mScanNodeId);
    std::fclose(o);
    return 0;
}
"""


def test_cpp_adapters_return_the_reference_peaks(tmp_path):
    L = 4
    src = tmp_path / "peaks.cpp"
    src.write_text(_CPP.replace("../my-lidar-graph-slam-v2_amd", os.path.join(ROOT, "my-lidar-graph-slam-v2_amd")))
    exe = tmp_path / "peaks"
    csrc = os.path.join(ROOT, "my-lidar-graph-slam-v2_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L" + csrc, "-lcsm_hip", "-Wl,-rpath," + csrc])
    c = synth.csm_case(0, rel_pose=(0.05, -0.02, 0.01))
    grid = np.ascontiguousarray(c["grid"], np.uint16)
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.array(grid.shape, np.int32).tobytes())
        f.write(np.array(c["geom"], np.float64).tobytes())
        f.write(np.array([len(c["angles"]), L], np.int32).tobytes())
        f.write(np.array(c["rel_pose"], np.float64).tobytes())
        f.write(np.array(c["init_pose"], np.float64).tobytes())
        f.write(np.array([RANGE[2]], np.float64).tobytes())
        f.write(grid.tobytes())
        f.write(np.asarray(c["angles"], np.float64).tobytes())
        f.write(np.asarray(c["ranges"], np.float64).tobytes())
    subprocess.check_call([str(exe), str(inp), str(outp)], timeout=120)
    v = np.frombuffer(outp.read_bytes(), np.float64)

    def rows(ref, win):
        return [PR.poses_of(r, win, c["rel_pose"])[1] + [r["score"], float(r["flags"])] for r in ref]

    ref, _, win = PR.peaks(c, *RANGE, L, K_MAX, EXCL)
    assert len(ref) == K_MAX and v[0] == K_MAX
    got = v[1:1 + 5 * (K_MAX + 1)].reshape(K_MAX + 1, 5).tolist()
    assert got[:K_MAX] == rows(ref, win)            # bit-exact doubles
    assert got[K_MAX] == got[0]                     # OptimizePose is the first peak
    v = v[1 + 5 * (K_MAX + 1):]
    dref, _, dwin = PR.peaks(c, *RANGE, L, K_MAX, EXCL, *DETECTOR_THR)
    assert 1 <= len(dref) and list(v[:3]) == [2.0, float(len(dref)), 2.0]
    got = v[3:3 + 5 * (len(dref) + 1)].reshape(len(dref) + 1, 5).tolist()
    assert got[:len(dref)] == rows(dref, dwin)
    assert got[len(dref)][:4] == got[0][:4] and got[len(dref)][4] == 9.0     # Detect: the first peak, its scan node id
