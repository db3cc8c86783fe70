/* adapter_demo.cpp -- drives the C++ adapters of csm_adapters.hpp from a
 * binary case file written by tests/test_gpu_adapter.py and prints one JSON
 * line. Built with g++ against libcsm_hip.so; exercises the same entry points a
 * reference-side ScanMatcher / LoopDetector subclass would.
 *
 * case file (little endian):
 *   int32 mode(0 csm, 1 bnb loop detector, 2 correlative loop detector, 3 grid search),
 *         rows, cols, n, n_queries, param_i (L or H)
 *   (mode 3 only: double step[3] right after the 8 doubles below)
 *   double res, offX, offY, rangeX, rangeY, rangeT, scoreThr, knownThr
 *   double rel[3]; double init[3 * n_queries]; double angles[n]; double ranges[n]
 *   uint16 grid[rows * cols]
 * mode 5 (pose-graph optimizer) has a layout of its own: see run_pose_graph.
 * mode 7 (pose sets) reads the common layout as: n_queries = robot poses in init, param_i = outputs of the
 *   resampling, rangeX = temperature, rangeY / rangeT = the low / high 32 bits of the resampling offset.
 * mode 8 (virtual scans) reads it as: n_queries = sensor poses in init, param_i = unknown_stops, rangeX =
 *   range_max, rangeY = range_min, rangeT = the sub-pixel scale, scoreThr = occupied_min; ranges is not used.
 */
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "csm_adapters.hpp"

using namespace CsmHip;

template <typename T>
static bool rd(FILE* f, T* p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }

/* mode 4: GridMapBuilderHIP + ScanMatcherCorrelativeHIP sharing one device
 * context. File: int32 4, n_nodes, n_beams, patch_size, n_latest, L;
 * double res, usable_min, usable_max, prob_hit, prob_miss, range_x, range_y, range_t;
 * double rel[3]; double init_local[3]; per node: double pose[3], min_range,
 * max_range, angles[n_beams], ranges[n_beams]. Builds the latest map, prints its
 * geometry and an FNV-1a hash of its cells, then matches the last node's scan. */
static int run_builder(FILE* f, const int32_t* hdr)
{
    const int nNodes = hdr[1], nBeams = hdr[2], patch = hdr[3], nLatest = hdr[4], lowRes = hdr[5];
    double prm[8], rel[3], init[3];
    if (!rd(f, prm, 8) || !rd(f, rel, 3) || !rd(f, init, 3))
        return 2;
    std::vector<std::vector<double>> angles(nNodes), ranges(nNodes);
    std::vector<ScanNodeView> nodes(nNodes);
    for (int k = 0; k < nNodes; ++k) {
        double head[5];
        angles[k].resize(nBeams);
        ranges[k].resize(nBeams);
        if (!rd(f, head, 5) || !rd(f, angles[k].data(), nBeams) || !rd(f, ranges[k].data(), nBeams))
            return 2;
        nodes[k].mNodeId = k;
        nodes[k].mGlobalPose = { head[0], head[1], head[2] };
        nodes[k].mMinRange = head[3];
        nodes[k].mMaxRange = head[4];
        nodes[k].mScanData.mAngles = angles[k].data();
        nodes[k].mScanData.mRanges = ranges[k].data();
        nodes[k].mScanData.mNumOfScans = nBeams;
        nodes[k].mScanData.mRelativeSensorPose = { rel[0], rel[1], rel[2] };
    }
    auto matcher = ScanMatcherCorrelativeHIP::Create("demo", lowRes, prm[5], prm[6], prm[7]);
    if (!matcher) {
        std::printf("{\"error\": \"no device\"}\n");
        return 3;
    }
    GridMapBuilderHIP builder(matcher->Context(), prm[0], patch, nLatest, prm[1], prm[2], prm[3], prm[4]);
    builder.UpdateLatestMap(nodes);
    const csm_map_build_info latestInfo = builder.LastBuildInfo();
    const GridMapView& map = builder.LatestMap();
    const std::vector<uint16_t> cells = builder.CopyLatestMapValues();
    uint64_t hash = 1469598103934665603ull;
    for (uint16_t v : cells) {
        hash = (hash ^ (v & 0xff)) * 1099511628211ull;
        hash = (hash ^ (v >> 8)) * 1099511628211ull;
    }
    ScanMatchingQuery q { map, nodes.back().mScanData, { init[0], init[1], init[2] } };
    const ScanMatchingSummary r = matcher->OptimizePose(q);
    /* a local map grown scan by scan (UpdateGridMap), its pose = the first node's */
    builder.CreateLocalMap(7);
    for (const ScanNodeView& nd : nodes)
        builder.UpdateGridMap(7, nodes.front().mGlobalPose, nd);
    const GridMapView local = builder.LocalMap(7);
    uint64_t localHash = 1469598103934665603ull;
    for (uint16_t v : builder.CopyLocalMapValues(7)) {
        localHash = (localHash ^ (v & 0xff)) * 1099511628211ull;
        localHash = (localHash ^ (v >> 8)) * 1099511628211ull;
    }
    std::printf("{\"rows\": %d, \"cols\": %d, \"off\": [\"%a\", \"%a\"], \"hash\": \"%016" PRIx64 "\", "
                "\"rays\": %lld, \"updates\": %lld, \"map_pose\": [\"%a\", \"%a\", \"%a\"], "
                "\"found\": %d, \"pose\": [\"%a\", \"%a\", \"%a\"], \"score\": \"%a\", "
                "\"local\": {\"rows\": %d, \"cols\": %d, \"off\": [\"%a\", \"%a\"], \"hash\": \"%016" PRIx64 "\"}}\n",
                map.mRows, map.mCols, map.mPosOffsetX, map.mPosOffsetY, hash,
                (long long)latestInfo.rays, (long long)latestInfo.cell_updates,
                builder.LatestMapPose().mX, builder.LatestMapPose().mY, builder.LatestMapPose().mTheta,
                r.mPoseFound ? 1 : 0, r.mEstimatedPose.mX, r.mEstimatedPose.mY, r.mEstimatedPose.mTheta,
                r.mScoreValue, local.mRows, local.mCols, local.mPosOffsetX, local.mPosOffsetY, localHash);
    return 0;
}

/* mode 5 (ConjugateGradient) or 6 (SchurCholesky): PoseGraphOptimizerLMHIP. File: int32 mode, n_local, n_scan, n_edges, iterations_max, loss_type;
 * double error_tolerance, loss_scale, initial_lambda; double local[3 n_local], scan[3 n_scan];
 * n_edges csm_pose_graph_edge records. Optimizes twice on one optimizer (the second call starts from
 * the first's poses and lambda) and prints the poses and lambda after each call. */
static int run_pose_graph(FILE* f, const int32_t* hdr)
{
    const int nl = hdr[1], ns = hdr[2], ne = hdr[3];
    double prm[3];
    std::vector<std::array<double, 3>> local(nl), scan(ns);
    std::vector<csm_pose_graph_edge> raw(ne);
    if (!rd(f, prm, 3) || !rd(f, local.data(), local.size()) || !rd(f, scan.data(), scan.size()) ||
        !rd(f, raw.data(), raw.size()))
        return 2;
    std::vector<EdgePose> edges;
    for (const csm_pose_graph_edge& r : raw) {
        EdgePose e {};
        e.mIsLoopConstraint = r.is_loop != 0;
        e.mLocalMapNodeIdx = r.local_map_index;
        e.mScanNodeIdx = r.scan_index;
        for (int j = 0; j < 3; ++j)
            e.mRelativePose[j] = r.relative_pose[j];
        for (int j = 0; j < 9; ++j)
            e.mInformationMat[j] = r.information[j];
        edges.push_back(e);
    }
    using Opt = PoseGraphOptimizerLMHIP;
    const bool cholRejected = !Opt::Create(Opt::SolverType::SparseCholesky, hdr[4], prm[0], prm[2], hdr[5], prm[1]);
    /* mode word 5: ConjugateGradient; 6: the same input and output with the direct SchurCholesky solver */
    const Opt::SolverType solver = hdr[0] == 6 ? Opt::SolverType::SchurCholesky : Opt::SolverType::ConjugateGradient;
    auto opt = Opt::Create(solver, hdr[4], prm[0], prm[2], hdr[5], prm[1]);
    if (!opt) {
        std::printf("{\"error\": \"no device\"}\n");
        return 3;
    }
    std::printf("{\"cholesky_rejected\": %d, \"calls\": [", cholRejected ? 1 : 0);
    for (int call = 0; call < 2; ++call) {
        opt->Optimize(local, scan, edges);
        std::printf("%s{\"lambda\": \"%a\", \"steps\": %d, \"poses\": [", call ? ", " : "", opt->Lambda(),
                    opt->LastInfo().steps);
        int k = 0;
        for (const auto* v : { &local, &scan })
            for (const auto& p : *v)
                std::printf("%s\"%a\", \"%a\", \"%a\"", k++ ? ", " : "", p[0], p[1], p[2]);
        std::printf("]}");
    }
    std::printf("]}\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2)
        return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f)
        return 2;
    int32_t hdr[6];
    double prm[8], rel[3];
    double step[3] = { 0.0, 0.0, 0.0 };
    if (!rd(f, hdr, 6))
        return 2;
    if (hdr[0] == 4 || hdr[0] == 5 || hdr[0] == 6) {
        const int rc = hdr[0] == 4 ? run_builder(f, hdr) : run_pose_graph(f, hdr);
        std::fclose(f);
        return rc;
    }
    if (false || !rd(f, prm, 8) || (hdr[0] == 3 && !rd(f, step, 3)) || !rd(f, rel, 3))
        return 2;
    const int mode = hdr[0], rows = hdr[1], cols = hdr[2], n = hdr[3], nq = hdr[4], pi = hdr[5];
    std::vector<double> init(3 * nq), angles(n), ranges(n);
    std::vector<uint16_t> grid((size_t)rows * cols);
    if (!rd(f, init.data(), init.size()) || !rd(f, angles.data(), n) || !rd(f, ranges.data(), n) ||
        !rd(f, grid.data(), grid.size()))
        return 2;
    std::fclose(f);

    GridMapView g;
    g.mValues = grid.data();
    g.mRows = rows;
    g.mCols = cols;
    g.mResolution = prm[0];
    g.mPosOffsetX = prm[1];
    g.mPosOffsetY = prm[2];
    ScanDataView s;
    s.mAngles = angles.data();
    s.mRanges = ranges.data();
    s.mNumOfScans = n;
    s.mRelativeSensorPose = { rel[0], rel[1], rel[2] };

    if (mode == 3) {
        auto m = ScanMatcherGridSearchHIP::Create("demo", prm[3], prm[4], prm[5], step[0], step[1], step[2]);
        if (!m) {
            std::printf("{\"error\": \"no device\"}\n");
            return 3;
        }
        ScanMatchingQuery q { g, s, { init[0], init[1], init[2] } };
        const ScanMatchingSummary r = m->OptimizePose(q, prm[6], prm[7]);
        std::printf("{\"found\": %d, \"pose\": [\"%a\", \"%a\", \"%a\"], \"score\": \"%a\", \"win\": [%d, %d, %d]}\n",
                    r.mPoseFound ? 1 : 0, r.mEstimatedPose.mX, r.mEstimatedPose.mY,
                    r.mEstimatedPose.mTheta, r.mScoreValue, r.mWinSizeX, r.mWinSizeY, r.mWinSizeTheta);
        return 0;
    }
    if (mode == 0) {
        auto m = ScanMatcherCorrelativeHIP::Create("demo", pi, prm[3], prm[4], prm[5]);
        if (!m) {
            std::printf("{\"error\": \"no device\"}\n");
            return 3;
        }
        ScanMatchingQuery q { g, s, { init[0], init[1], init[2] } };
        /* CSM_DEMO_PRIOR="xx,yy,tt": a diagonal motion prior on the offset from the initial pose */
        if (const char* e = std::getenv("CSM_DEMO_PRIOR")) {
            double information[9] = { 0 };
            if (std::sscanf(e, "%lf,%lf,%lf", &information[0], &information[4], &information[8]) != 3)
                return 2;
            m->UseMotionPrior(information);
        }
        const ScanMatchingSummary r = (prm[6] == 0.0 && prm[7] == 0.0)
                                          ? m->OptimizePose(q)
                                          : m->OptimizePose(q, prm[6], prm[7]);
        if (std::getenv("CSM_DEMO_PRIOR")) {
            const csm_prior_result& p = m->LastPriorResult();
            std::fprintf(stderr, "prior: winner (%d, %d, %d) paid %lld key units; unweighted (%d, %d, %d)\n",
                         p.best.best_x, p.best.best_y, p.best.best_theta, (long long)p.penalty,
                         p.unweighted.best_x, p.unweighted.best_y, p.unweighted.best_theta);
        }
        int metricIds = 0;
        ReportScanMatcherMetrics(m->Name(), r, s.mNumOfScans, [&](const std::string& id, double) {
            metricIds += id.rfind("demo.", 0) == 0;
        });
        if (metricIds != 15)
            return 4;
        std::printf("{\"found\": %d, \"pose\": [\"%a\", \"%a\", \"%a\"], \"score\": \"%a\", \"win\": [%d, %d, %d]}\n",
                    r.mPoseFound ? 1 : 0, r.mEstimatedPose.mX, r.mEstimatedPose.mY,
                    r.mEstimatedPose.mTheta, r.mScoreValue, r.mWinSizeX, r.mWinSizeY, r.mWinSizeTheta);
        return 0;
    }
    if (mode == 7) {
        /* ScorePixelAccurateHIP at one robot pose and at all of them, ParticleSetHIP on the same context */
        auto scorer = ScorePixelAccurateHIP::Create();
        if (!scorer) {
            std::printf("{\"error\": \"no device\"}\n");
            return 3;
        }
        g.mId = 42;
        scorer->Upload(g);
        const csm_geometry geom = { g.mResolution, g.mPosOffsetX, g.mPosOffsetY };
        std::vector<RobotPose2D<double>> robot(nq);
        for (int i = 0; i < nq; ++i)
            robot[i] = { init[3 * i], init[3 * i + 1], init[3 * i + 2] };
        const std::vector<RobotPose2D<double>> sensor = ScorePixelAccurateHIP::SensorPoses(s, robot);
        const ScoreSummary one = scorer->Score(g.mId, geom, s, sensor.front());
        const std::vector<ScoreSummary> all = scorer->ScoreManyRobotPoses(g.mId, geom, s, robot);
        ParticleSetHIP particles(scorer->Context(), prm[3], prm[7]);
        const std::uint64_t offset = ((std::uint64_t)prm[5] << 32) | (std::uint64_t)prm[4];
        const ParticleSetHIP::Update u = particles.MeasurementUpdate(g.mId, geom, s, sensor, (size_t)pi, offset);
        std::printf("{\"one\": [%u, %u, \"%a\", \"%a\", \"%a\"], \"all\": [", one.mSumValues, one.mKnown,
                    one.mNormalizedScore, one.mScore, one.mKnownRate);
        for (size_t i = 0; i < all.size(); ++i)
            std::printf("%s[%u, %u, \"%a\", \"%a\", \"%a\"]", i ? ", " : "", all[i].mSumValues, all[i].mKnown,
                        all[i].mNormalizedScore, all[i].mScore, all[i].mKnownRate);
        std::printf("], \"weights\": [");
        for (size_t i = 0; i < u.mWeights.size(); ++i)
            std::printf("%s%u", i ? ", " : "", u.mWeights[i]);
        std::printf("], \"ancestors\": [");
        for (size_t i = 0; i < u.mAncestors.size(); ++i)
            std::printf("%s%d", i ? ", " : "", u.mAncestors[i]);
        std::printf("], \"ess\": \"%a\", \"m0\": %llu, \"key_max\": %llu, \"best_index\": %d, \"support\": %d, "
                    "\"bin_shift\": %d, \"found\": %d, \"uncertain\": %d}\n", u.mEffectiveSampleSize,
                    (unsigned long long)u.mUpdate.m0, (unsigned long long)u.mUpdate.key_max, u.mUpdate.best_index,
                    u.mUpdate.support, u.mUpdate.bin_shift, u.mUpdate.found, u.mInfo.uncertain_poses);
        return 0;
    }
    if (mode == 8) {
        /* VirtualScanHIP: the records and ranges of every pose's beams, and the scan of the first pose */
        auto caster = VirtualScanHIP::Create();
        if (!caster) {
            std::printf("{\"error\": \"no device\"}\n");
            return 3;
        }
        g.mId = 42;
        caster->Upload(g);
        const csm_geometry geom = { g.mResolution, g.mPosOffsetX, g.mPosOffsetY };
        std::vector<RobotPose2D<double>> sensor(nq);
        for (int i = 0; i < nq; ++i)
            sensor[i] = { init[3 * i], init[3 * i + 1], init[3 * i + 2] };
        RayCastSettings settings;
        settings.mRangeMax = prm[3];
        settings.mRangeMin = prm[4];
        settings.mSubpixelScale = (int)prm[5];
        settings.mOccupiedMin = (std::uint32_t)prm[6];
        settings.mUnknownStops = pi != 0;
        settings.mNoneValue = -1.0;
        const VirtualScanHIP::Casts casts = caster->Cast(g.mId, geom, sensor, angles, settings);
        const VirtualScan scan = caster->ScanFromMap(g.mId, geom, sensor.front(), angles, settings);
        std::printf("{\"records\": [");
        for (size_t i = 0; i < casts.mRecords.size(); ++i) {
            const csm_ray_cast_record& r = casts.mRecords[i];
            std::printf("%s[%d, %d, %u, %d, %lld, \"%a\"]", i ? ", " : "", r.cell_x, r.cell_y, r.value, r.kind,
                        (long long)r.dist2, casts.mRanges[i]);
        }
        std::printf("], \"scan\": [");
        for (size_t i = 0; i < scan.mAngles.size(); ++i)
            std::printf("%s[\"%a\", \"%a\"]", i ? ", " : "", scan.mAngles[i], scan.mRanges[i]);
        std::printf("], \"rays\": %lld, \"beams\": %zu}\n", (long long)casts.mInfo.rays, scan.View().mNumOfScans);
        return 0;
    }
    /* CSM_DEMO_DEVICES="0,0": the detector over a device list (here two members on GPU 0) */
    std::vector<int> devices;
    if (const char* e = std::getenv("CSM_DEMO_DEVICES"))
        for (const char* p = e; *p;) {
            devices.push_back(std::atoi(p));
            while (*p && *p != ',')
                ++p;
            if (*p == ',')
                ++p;
        }
    if (devices.empty())
        devices.push_back(0);
    auto d = mode == 1 ? LoopDetectorBranchBoundHIP::Create("demo", pi, prm[3], prm[4], prm[5], prm[6], prm[7],
                                                            devices)
                       : nullptr;
    auto dc = mode == 2 ? LoopDetectorCorrelativeHIP::Create("demo", pi, prm[3], prm[4], prm[5], prm[6], prm[7])
                        : nullptr;
    if (!d && !dc) {
        std::printf("{\"error\": \"no device\"}\n");
        return 3;
    }
    const bool refine = std::getenv("CSM_DEMO_REFINE") != nullptr;   /* the detector's final matcher */
    if (d && refine)
        d->UseFinalScanMatcher();
    g.mId = 42;
    LoopDetectionQueryVector qs;
    for (int i = 0; i < nq; ++i) {
        LoopDetectionQuery q;
        q.mReferenceLocalMap = g;
        q.mQueryScanData = s;
        /* local map node at the origin: the scan node's global pose is its map-local pose */
        q.mReferenceLocalMapNodeGlobalPose = { 0.0, 0.0, 0.0 };
        q.mQueryScanNodeGlobalPose = { init[3 * i], init[3 * i + 1], init[3 * i + 2] };
        q.mQueryScanNodeId = i;
        qs.push_back(q);
    }
    const LoopDetectionResultVector rs = d ? d->Detect(qs) : dc->Detect(qs);
    std::printf("{\"results\": [");
    for (size_t i = 0; i < rs.size(); ++i)
        std::printf("%s{\"node\": %d, \"pose\": [\"%a\", \"%a\", \"%a\"], \"score\": \"%a\", "
                    "\"cost\": \"%a\", \"cov00\": \"%a\"}", i ? ", " : "",
                    rs[i].mScanNodeId, rs[i].mRelativePose.mX, rs[i].mRelativePose.mY,
                    rs[i].mRelativePose.mTheta, rs[i].mScoreValue, rs[i].mNormalizedCost,
                    rs[i].mEstimatedCovariance[0]);
    std::printf("]}\n");
    return 0;
}
