/* csm_adapters.hpp -- header-only C++17 host side above the C ABI
 * (include/csm_hip.h). Mirrors the reference's plugin interfaces for the hot
 * path with the same names, argument meaning and error behaviour:
 *
 *   ScanMatcherCorrelativeHIP   <- ScanMatcherCorrelative
 *        inc/mapping/scan_matcher_correlative.hpp:53-125, scan_matcher.hpp:89-117
 *   LoopDetectorBranchBoundHIP  <- LoopDetectorBranchBound (search part)
 *        inc/mapping/loop_detector_branch_bound.hpp:71-112, loop_detector.hpp:97-116
 *   LoopDetectorCorrelativeHIP  <- LoopDetectorCorrelative (search part)
 *        inc/mapping/loop_detector_correlative.hpp, src/mapping/loop_detector_correlative.cpp:59-156
 *   ScanMatcherGridSearchHIP    <- ScanMatcherGridSearch
 *        inc/mapping/scan_matcher_grid_search.hpp, src/mapping/scan_matcher_grid_search.cpp:69-190
 *   GridMapBuilderHIP           <- GridMapBuilder (latest-map part)
 *        inc/mapping/grid_map_builder.hpp, src/mapping/grid_map_builder.cpp:497-527, 561-695
 *   ScorePixelAccurateHIP       <- ScorePixelAccurate (ScoreFunction::Score at free poses)
 *        inc/mapping/score_function.hpp:29-60, src/mapping/score_function_pixel_accurate.cpp:16-58
 *   ParticleSetHIP              (beyond the reference) weights and resampling of a particle set
 *   VirtualScanHIP              (beyond the reference) beams cast through a resident map: records, ranges, a scan
 *   LoopSearcherNearestHIP      <- LoopSearcherNearest
 *        inc/mapping/loop_searcher_nearest.hpp:33-63, src/mapping/loop_searcher_nearest.cpp:59-170
 *   LoopSearcherAppearanceHIP   (no counterpart: candidates by scan descriptors, csm_appearance_search)
 *
 * The reference headers cannot be included in this image (Eigen3 / Boost are
 * absent), so the few value types the interfaces use are restated here in
 * namespace CsmHip. INTEGRATION.md shows the ~40-line glue a maintainer adds
 * inside the reference tree to derive these from the real
 * MyLidarGraphSlam::Mapping::ScanMatcher / LoopDetector.
 *
 * Error convention: like the reference's Assert() (inc/util.hpp:38-72) a
 * failed C-ABI call prints csm_last_error() with file:line and abort()s;
 * device-initialisation failure is reported from Create() as a null pointer,
 * like LoadBitstream's bool (src/slam_launcher.cpp:83-107).
 */
#ifndef CSM_ADAPTERS_HPP
#define CSM_ADAPTERS_HPP

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <numeric>
#include <set>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "csm_hip.h"

namespace CsmHip {

#define CSM_ASSERT_OK(ctx, expr)                                                   \
    do {                                                                           \
        const int rc_ = (expr);                                                    \
        if (rc_ != 0) {                                                            \
            std::fprintf(stderr, "Assertion failed: %s == 0 (rc %d: %s) at %s:%d\n", \
                         #expr, rc_, csm_last_error(ctx), __FILE__, __LINE__);     \
            std::abort();                                                          \
        }                                                                          \
    } while (0)

/* a condition of the adapters' own: CSM_ASSERT_THAT(cond, "text" [, printf arguments of the text]) */
#define CSM_ASSERT_THAT(cond, ...)                                                 \
    do {                                                                           \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "Assertion failed: ");                            \
            std::fprintf(stderr, __VA_ARGS__);                                     \
            std::fprintf(stderr, " at %s:%d\n", __FILE__, __LINE__);               \
            std::abort();                                                          \
        }                                                                          \
    } while (0)

/* inc/pose.hpp:17-46 */
template <typename T>
struct RobotPose2D {
    T mX, mY, mTheta;
};

/* What a matcher reads of GridMap (inc/grid_map_new/grid_map.hpp): the dense
 * export of CopyValues (src/grid_map_new/grid_map.cpp:439-457) plus geometry
 * (inc/grid_map_new/grid_map_geometry.hpp:228-240). mId plays LocalMapId::mId;
 * kInvalidId marks a throw-away map (the frontend's latest map), as
 * LocalMapId::Invalid does in scan_matcher_correlative_fpga.cpp:177-184. */
struct GridMapView {
    static constexpr std::uint64_t kInvalidId = ~0ull;
    /* ids from here on are the adapters' own (throw-away maps): a caller's id must be smaller */
    static constexpr std::uint64_t kReservedIds = 1ull << 62;
    /* the likelihood field of map id m lives under m | kLikelihoodIdBit (ScanMatcherCorrelativeHIP::
     * UseLikelihoodField): callers' ids and the adapters' throw-away ids both leave bit 63 clear */
    static constexpr std::uint64_t kLikelihoodIdBit = 1ull << 63;
    /* ... and its distance field under m | kDistanceIdBit (UseDistanceField), for a caller's id m. The
     * adapters' throw-away ids carry this bit already: FieldId */
    static constexpr std::uint64_t kDistanceIdBit = 1ull << 62;
    /* Where the field of map id `id` lies: id | bit; a throw-away map's field, of either kind, under bit 63
     * (a matcher has one kind of field, and a throw-away map's field goes with it when the call ends). */
    static constexpr std::uint64_t FieldId(std::uint64_t id, std::uint64_t bit)
    {
        return id | ((id & bit) ? kLikelihoodIdBit : bit);
    }
    const std::uint16_t* mValues = nullptr;   /* row-major rows*cols */
    int mRows = 0, mCols = 0;
    double mResolution = 0.0;
    double mPosOffsetX = 0.0, mPosOffsetY = 0.0;
    std::uint64_t mId = kInvalidId;
    /* A map with an id is uploaded once and then read from the device (the
     * reference caches by LocalMapId because finished local maps never change,
     * loop_detector_branch_bound.hpp:98). A caller that passes a map which is
     * still growing under an id bumps mRevision whenever its cells change: the
     * adapters upload again when the revision differs from the one they hold. */
    std::uint64_t mRevision = 0;
};

/* What a matcher reads of Sensor::ScanData<double>
 * (inc/sensor/sensor_data.hpp:63-185) */
struct ScanDataView {
    const double* mAngles = nullptr;
    const double* mRanges = nullptr;
    std::size_t mNumOfScans = 0;
    RobotPose2D<double> mRelativeSensorPose { 0.0, 0.0, 0.0 };
};

/* inc/mapping/scan_matcher.hpp:27-50 */
struct ScanMatchingQuery {
    GridMapView mGridMap;
    ScanDataView mScanData;
    RobotPose2D<double> mMapLocalInitialPose;
};

/* inc/mapping/scan_matcher.hpp:53-82. Cost and covariance come from the
 * caller's CostFunction (scan_matcher_correlative.cpp:209-219): pass a
 * callback, or leave them zero. */
struct ScanMatchingSummary {
    bool mPoseFound = false;
    double mNormalizedCost = 0.0;
    RobotPose2D<double> mMapLocalInitialPose { 0, 0, 0 };
    RobotPose2D<double> mEstimatedPose { 0, 0, 0 };
    double mEstimatedCovariance[9] = { 0 };
    /* extras the reference observes as metrics
     * (scan_matcher_correlative.cpp:222-236) */
    RobotPose2D<double> mBestSensorPose { 0, 0, 0 };
    double mScoreValue = 0.0;
    int mWinSizeX = 0, mWinSizeY = 0, mWinSizeTheta = 0;
    double mStepSizeX = 0, mStepSizeY = 0, mStepSizeTheta = 0;
    double mInputSetupTime = 0, mOptimizationTime = 0;   /* micro seconds */
    long long mNumOfCandidates = 0;
    std::uint32_t mFlags = 0;
};

/* Cost / covariance hook: void(query, bestSensorPose, &normalizedCost, cov[9]) */
using CostCallback = void (*)(const ScanMatchingQuery&, const RobotPose2D<double>&, double*,
                              double*);

/* What the map update reads of a ScanNode (inc/mapping/pose_graph.hpp) and its
 * ScanData (inc/sensor/sensor_data.hpp:63-185) */
struct ScanNodeView {
    int mNodeId = 0;
    RobotPose2D<double> mGlobalPose { 0.0, 0.0, 0.0 };
    ScanDataView mScanData;
    double mMinRange = 0.0, mMaxRange = 0.0;
};

namespace detail {
/* which revision of which map id a context holds */
using RevisionMap = std::map<std::uint64_t, std::uint64_t>;

/* The residency rule of a matcher's query map, for all matchers: the map of a query lies on the device under
 * its own id, uploaded when the context does not hold it or holds another revision of it; a map without an id
 * (kInvalidId: a throw-away map) is uploaded on every call under the matcher's reserved id and released when
 * the call ends. A view without cells (mValues == nullptr) uploads nothing: the map is already resident, e.g.
 * built by a GridMapBuilderHIP on this context. */
class ResidentQueryMaps final {
public:
    /* One call's use of a query map: Id() is where its cells lie on the device. Its end is the end of the
     * call: a throw-away map that was uploaded is released, and after it what was derived from it. */
    class Use final {
    public:
        Use(csm_ctx* ctx, std::uint64_t id, bool temporary, bool release) :
            mCtx(ctx), mId(id), mTemporary(temporary), mRelease { id, 0 }, mNumOfReleases(release ? 1 : 0) { }
        Use(Use&& other) : Use(static_cast<const Use&>(other)) { other.mNumOfReleases = 0; }
        Use& operator=(const Use&) = delete;
        ~Use()
        {
            for (int i = 0; i < this->mNumOfReleases; ++i)
                CSM_ASSERT_OK(this->mCtx, csm_release_grid(this->mCtx, this->mRelease[i]));
        }

        std::uint64_t Id() const { return this->mId; }
        bool Temporary() const { return this->mTemporary; }
        /* derivedId holds a map made from this one (a likelihood field): it goes when this one goes */
        void ReleaseWithIt(std::uint64_t derivedId)
        {
            if (this->mNumOfReleases == 1)
                this->mRelease[this->mNumOfReleases++] = derivedId;
        }

    private:
        Use(const Use&) = default;          /* for the move alone, which takes the releases with it */
        csm_ctx* mCtx;
        std::uint64_t mId;
        bool mTemporary;
        std::uint64_t mRelease[2];
        int mNumOfReleases;
    };

    /* throwAwayId: GridMapView::kReservedIds + 0 / 1 / 2, one per matcher class */
    ResidentQueryMaps(csm_ctx* ctx, std::uint64_t throwAwayId) : mCtx(ctx), mThrowAwayId(throwAwayId) { }

    Use Acquire(const GridMapView& g)
    {
        const bool temporary = g.mId == GridMapView::kInvalidId;
        CSM_ASSERT_THAT(temporary || g.mId < GridMapView::kReservedIds, "map id below 2^62");
        const std::uint64_t id = temporary ? this->mThrowAwayId : g.mId;
        auto held = this->mRevisions.find(id);
        if (g.mValues && (temporary || !csm_has_grid(this->mCtx, id) || held == this->mRevisions.end() ||
                          held->second != g.mRevision)) {
            CSM_ASSERT_OK(this->mCtx, csm_upload_grid(this->mCtx, id, g.mValues, g.mRows, g.mCols));
            this->mRevisions[id] = g.mRevision;
        }
        return Use(this->mCtx, id, temporary, temporary && g.mValues != nullptr);
    }

private:
    csm_ctx* mCtx;
    const std::uint64_t mThrowAwayId;
    RevisionMap mRevisions;
};

struct CtxDeleter {
    void operator()(csm_ctx* c) const { if (c) csm_destroy(c); }
};
using CtxPtr = std::unique_ptr<csm_ctx, CtxDeleter>;

inline CtxPtr MakeContext(int deviceId)
{
    csm_config cfg {};
    cfg.device_id = deviceId;
    csm_ctx* raw = nullptr;
    if (csm_create(&cfg, &raw) != 0)
        return CtxPtr();
    return CtxPtr(raw);
}

/* a context of the adapter's own, or one that another adapter owns (and keeps alive) */
class ContextRef final {
public:
    explicit ContextRef(CtxPtr owned) : mOwned(std::move(owned)) { }
    explicit ContextRef(csm_ctx* shared) : mShared(shared) { }
    csm_ctx* Get() const { return this->mOwned ? this->mOwned.get() : this->mShared; }

private:
    CtxPtr mOwned;
    csm_ctx* mShared = nullptr;
};

inline csm_scan ToScan(const ScanDataView& s)
{
    csm_scan out {};
    out.angles = s.mAngles;
    out.ranges = s.mRanges;
    out.n_points = static_cast<std::int32_t>(s.mNumOfScans);
    out.relative_sensor_pose[0] = s.mRelativeSensorPose.mX;
    out.relative_sensor_pose[1] = s.mRelativeSensorPose.mY;
    out.relative_sensor_pose[2] = s.mRelativeSensorPose.mTheta;
    return out;
}

inline csm_scan_node ToScanNode(const ScanNodeView& n)
{
    csm_scan_node out {};
    out.global_pose[0] = n.mGlobalPose.mX;
    out.global_pose[1] = n.mGlobalPose.mY;
    out.global_pose[2] = n.mGlobalPose.mTheta;
    out.scan = ToScan(n.mScanData);
    out.min_range = n.mMinRange;
    out.max_range = n.mMaxRange;
    return out;
}

inline std::vector<csm_scan_node> ToScanNodes(const ScanNodeView* nodes, std::size_t numOfNodes)
{
    std::vector<csm_scan_node> flat(numOfNodes);
    for (std::size_t i = 0; i < numOfNodes; ++i)
        flat[i] = ToScanNode(nodes[i]);
    return flat;
}

/* geometry + id of a map whose cells live on the device */
inline GridMapView ToView(const csm_map_shape& shape, std::uint64_t id)
{
    GridMapView view;
    view.mRows = shape.rows;
    view.mCols = shape.cols;
    view.mResolution = shape.resolution;
    view.mPosOffsetX = shape.offset_x;
    view.mPosOffsetY = shape.offset_y;
    view.mId = id;
    return view;
}

/* the scan of `scan` against the map that lies under `id` on the device with g's geometry, at the map-local
 * robot pose `pose`, as the batch entries, the cost entries and the ray check take it */
inline csm_loop_query ToLoopQuery(std::uint64_t id, const GridMapView& g, const ScanDataView& scan,
                                  const RobotPose2D<double>& pose)
{
    csm_loop_query f {};
    f.map_id = id;
    f.geometry = { g.mResolution, g.mPosOffsetX, g.mPosOffsetY };
    f.scan = ToScan(scan);
    f.initial_pose[0] = pose.mX;
    f.initial_pose[1] = pose.mY;
    f.initial_pose[2] = pose.mTheta;
    return f;
}

inline csm_pose_set ToPoseSet(std::uint64_t mapId, const csm_geometry& geometry, const ScanDataView& scan,
                              const std::vector<RobotPose2D<double>>& mapLocalSensorPoses)
{
    /* RobotPose2D<double> is three contiguous doubles: the vector is the flat pose array */
    static_assert(sizeof(RobotPose2D<double>) == 3 * sizeof(double), "pose layout");
    csm_pose_set set {};
    set.map_id = mapId;
    set.geometry = geometry;
    set.scan = ToScan(scan);
    set.poses = mapLocalSensorPoses.empty() ? nullptr : &mapLocalSensorPoses.front().mX;
    set.n_poses = static_cast<std::int32_t>(mapLocalSensorPoses.size());
    return set;
}

inline csm_correlative_params CorrelativeParams(double rangeX, double rangeY, double rangeTheta, int lowResolution,
                                                double normalizedScoreThreshold, double knownRateThreshold)
{
    csm_correlative_params prm {};
    prm.range_x = rangeX;
    prm.range_y = rangeY;
    prm.range_theta = rangeTheta;
    prm.low_resolution = lowResolution;
    prm.score_threshold = normalizedScoreThreshold;
    prm.known_rate_threshold = knownRateThreshold;
    return prm;
}

inline void FillSummary(const csm_summary& s, const RobotPose2D<double>& initial,
                        ScanMatchingSummary* out)
{
    out->mPoseFound = s.pose_found != 0;
    out->mMapLocalInitialPose = initial;
    out->mEstimatedPose = { s.estimated_pose[0], s.estimated_pose[1], s.estimated_pose[2] };
    out->mBestSensorPose = { s.best_sensor_pose[0], s.best_sensor_pose[1], s.best_sensor_pose[2] };
    out->mScoreValue = s.raw.score;
    out->mWinSizeX = s.win_x;
    out->mWinSizeY = s.win_y;
    out->mWinSizeTheta = s.win_theta;
    out->mStepSizeX = s.step_x;
    out->mStepSizeY = s.step_y;
    out->mStepSizeTheta = s.step_theta;
    out->mInputSetupTime = s.input_setup_us;
    out->mOptimizationTime = s.optimization_us;
    out->mNumOfCandidates = s.candidates;
    out->mFlags = s.raw.flags;
}
/* CostSquareError::Cost / n and ComputeCovariance at the best sensor pose on the device
 * (scan_matcher_correlative.cpp:209-219) */
inline void DeviceSquareErrorCost(csm_ctx* ctx, const csm_loop_query& query, const double bestSensorPose[3],
                                  double covarianceScale, ScanMatchingSummary* out)
{
    csm_refine_result r {};
    CSM_ASSERT_OK(ctx, csm_cost_covariance_batch(ctx, &query, 1, bestSensorPose, covarianceScale, &r));
    out->mNormalizedCost = r.normalized_cost;
    for (int c = 0; c < 9; ++c)
        out->mEstimatedCovariance[c] = r.covariance[c];
}
/* CostGreedyEndpoint::Cost / n and ComputeCovariance at the best sensor pose on the device
 * (scan_matcher_correlative.cpp:209-219 with a "GreedyEndpoint" cost) */
inline void DeviceGreedyCost(csm_ctx* ctx, const csm_loop_query& query, const double bestSensorPose[3],
                             const csm_greedy_params& prm, ScanMatchingSummary* out)
{
    csm_hill_climbing_result r {};
    CSM_ASSERT_OK(ctx, csm_greedy_cost_covariance_batch(ctx, &query, 1, bestSensorPose, &prm, &r));
    out->mNormalizedCost = r.normalized_cost;
    for (int c = 0; c < 9; ++c)
        out->mEstimatedCovariance[c] = r.covariance[c];
}
} /* namespace detail */

/* The 15 value sequences a matcher registers with the MetricManager and observes
 * once per call (src/mapping/scan_matcher_correlative.cpp:37-70, 222-236), under
 * the same ids: observe("<matcherName>.InputSetupTime", value), ... Ignored /
 * processed nodes lose their meaning when every candidate is scored: reported
 * as 0 and the number of candidates. The glue in the reference tree passes
 * [&](const std::string& id, double v) { its ValueSequence for id ->Observe(v); }. */
template <typename Observe>
inline void ReportScanMatcherMetrics(const std::string& matcherName, const ScanMatchingSummary& s,
                                     std::size_t numOfScans, Observe&& observe)
{
    const double dx = s.mEstimatedPose.mX - s.mMapLocalInitialPose.mX;
    const double dy = s.mEstimatedPose.mY - s.mMapLocalInitialPose.mY;
    observe(matcherName + ".InputSetupTime", s.mInputSetupTime);
    observe(matcherName + ".OptimizationTime", s.mOptimizationTime);
    observe(matcherName + ".DiffTranslation", std::sqrt(dx * dx + dy * dy));
    observe(matcherName + ".DiffRotation", std::abs(s.mMapLocalInitialPose.mTheta - s.mEstimatedPose.mTheta));
    observe(matcherName + ".WinSizeX", static_cast<double>(s.mWinSizeX));
    observe(matcherName + ".WinSizeY", static_cast<double>(s.mWinSizeY));
    observe(matcherName + ".WinSizeTheta", static_cast<double>(s.mWinSizeTheta));
    observe(matcherName + ".StepSizeX", s.mStepSizeX);
    observe(matcherName + ".StepSizeY", s.mStepSizeY);
    observe(matcherName + ".StepSizeTheta", s.mStepSizeTheta);
    observe(matcherName + ".NumOfIgnoredNodes", 0.0);
    observe(matcherName + ".NumOfProcessedNodes", static_cast<double>(s.mNumOfCandidates));
    observe(matcherName + ".ScoreValue", static_cast<double>(static_cast<float>(s.mScoreValue)));   /* a float sequence */
    observe(matcherName + ".CostValue", s.mNormalizedCost);
    observe(matcherName + ".NumOfScans", static_cast<double>(numOfScans));
}

class ScanMatcherCorrelativeHIP final {
public:
    /* Constructor arguments as ScanMatcherCorrelative
     * (inc/mapping/scan_matcher_correlative.hpp:58-66); Create() returns null
     * when no usable GPU exists. */
    static std::unique_ptr<ScanMatcherCorrelativeHIP> Create(
        const std::string& scanMatcherName, int lowResolution, double rangeX, double rangeY,
        double rangeTheta, CostCallback costFunc = nullptr, int deviceId = 0)
    {
        detail::CtxPtr ctx = detail::MakeContext(deviceId);
        if (!ctx)
            return nullptr;
        return std::unique_ptr<ScanMatcherCorrelativeHIP>(new ScanMatcherCorrelativeHIP(
            scanMatcherName, lowResolution, rangeX, rangeY, rangeTheta, costFunc, std::move(ctx)));
    }

    ScanMatcherCorrelativeHIP(const ScanMatcherCorrelativeHIP&) = delete;
    ScanMatcherCorrelativeHIP& operator=(const ScanMatcherCorrelativeHIP&) = delete;

    const std::string& Name() const { return this->mName; }
    /* the device context, to share resident maps with a GridMapBuilderHIP */
    csm_ctx* Context() const { return this->mCtx.get(); }

    /* ScanMatcher::OptimizePose (scan_matcher_correlative.cpp:92-115): the whole
     * window, thresholds 0.0 / 0.0 */
    ScanMatchingSummary OptimizePose(const ScanMatchingQuery& queryInfo)
    {
        return this->OptimizePose(queryInfo, 0.0, 0.0);
    }

    /* The 6-argument overload the loop detectors call
     * (scan_matcher_correlative.cpp:118-244); the coarse map is built and cached
     * on the device instead of being passed in. */
    ScanMatchingSummary OptimizePose(const ScanMatchingQuery& q,
                                     const double normalizedScoreThreshold,
                                     const double knownRateThreshold)
    {
        csm_ctx* ctx = this->mCtx.get();
        Search w = this->Prepare(q, normalizedScoreThreshold, knownRateThreshold);
        const csm_loop_query& f = w.mQuery;
        /* the search runs on the likelihood field when one is asked for; cost, covariance and any
         * refinement below stay on the occupancy map f.map_id, which they are bilinear in */
        const std::uint64_t searchId =
            this->mLikelihoodSigma > 0.0 || this->mDistanceSigma > 0.0 ? this->MakeField(q.mGridMap, w.mMap) : f.map_id;
        csm_summary s {};
        if (this->mUsePrior) {
            /* the winner under the motion prior; the unweighted one stays in LastPriorResult() */
            csm_prior_summary v {};
            CSM_ASSERT_OK(ctx, csm_correlative_match_prior(ctx, searchId, &f.geometry, &f.scan, f.initial_pose,
                                                           &w.mParams, &this->mPrior, &v));
            s = v.summary;
            this->mLastPrior = v.prior;
        } else {
            CSM_ASSERT_OK(ctx, csm_correlative_match(ctx, searchId, &f.geometry, &f.scan, f.initial_pose, &w.mParams,
                                                     &s));
        }
        ScanMatchingSummary out;
        detail::FillSummary(s, q.mMapLocalInitialPose, &out);
        if (this->mCostFunc)
            this->mCostFunc(q, out.mBestSensorPose, &out.mNormalizedCost, out.mEstimatedCovariance);
        else if (this->mDeviceCovarianceScale > 0.0)
            detail::DeviceSquareErrorCost(ctx, f, s.best_sensor_pose, this->mDeviceCovarianceScale, &out);
        else if (this->mUseDeviceGreedy)
            detail::DeviceGreedyCost(ctx, f, s.best_sensor_pose, this->mGreedy, &out);
        return out;
    }

    /* The K best DISTINCT poses of the window, best first (csm_correlative_peaks; beyond the reference,
     * which keeps scoreMax only): a second entry scoring close to the first is a perceptually aliased
     * match. exclX / exclY / exclTheta: half-widths, in search steps, of the box around a chosen pose
     * in which no later one is taken. Cost and covariance are left zero. */
    std::vector<ScanMatchingSummary> OptimizePosePeaks(const ScanMatchingQuery& q, int numOfPeaks, int exclX,
                                                       int exclY, int exclTheta,
                                                       const double normalizedScoreThreshold = 0.0,
                                                       const double knownRateThreshold = 0.0)
    {
        csm_ctx* ctx = this->mCtx.get();
        const Search w = this->Prepare(q, normalizedScoreThreshold, knownRateThreshold);
        const csm_loop_query& f = w.mQuery;
        const csm_peaks_params peaks { numOfPeaks, exclX, exclY, exclTheta, 0 };
        csm_summary s[CSM_PEAKS_MAX] {};
        std::int32_t n = 0;
        CSM_ASSERT_OK(ctx, csm_correlative_peaks(ctx, f.map_id, &f.geometry, &f.scan, f.initial_pose, &w.mParams,
                                                 &peaks, s, &n));
        std::vector<ScanMatchingSummary> out(static_cast<std::size_t>(n));
        for (std::int32_t j = 0; j < n; ++j)
            detail::FillSummary(s[j], q.mMapLocalInitialPose, &out[j]);
        return out;
    }

    /* OptimizePose with mEstimatedCovariance read off the window's whole score volume
     * (csm_correlative_covariance; beyond the reference, whose covariance is the cost function's Hessian at
     * the winner): every candidate weighs exp(-(best score - score) / temperature), so a ridge, a plateau
     * or a second lobe in the window widens the matrix. temperature: in score units, the caller's choice.
     * *borderSupport (optional): weighted candidates on a face of the window; non-zero says the window
     * truncated the distribution. The cost stays zero. */
    ScanMatchingSummary OptimizePoseVolumeCovariance(const ScanMatchingQuery& q, double temperature,
                                                     long long* borderSupport = nullptr,
                                                     const double normalizedScoreThreshold = 0.0,
                                                     const double knownRateThreshold = 0.0)
    {
        csm_ctx* ctx = this->mCtx.get();
        const Search w = this->Prepare(q, normalizedScoreThreshold, knownRateThreshold);
        const csm_loop_query& f = w.mQuery;
        const csm_volume_params volume { temperature, 0 };
        csm_volume_summary v {};
        CSM_ASSERT_OK(ctx, csm_correlative_covariance(ctx, f.map_id, &f.geometry, &f.scan, f.initial_pose, &w.mParams,
                                                      &volume, &v));
        ScanMatchingSummary out;
        detail::FillSummary(v.summary, q.mMapLocalInitialPose, &out);
        for (int c = 0; c < 9; ++c)
            out.mEstimatedCovariance[c] = v.covariance[c];
        if (borderSupport)
            *borderSupport = v.moments.border_support;
        return out;
    }

    /* Cost and covariance from the device's CostSquareError instead of a host callback
     * ("CovarianceScale", launcher_settings_default.json:11-13). */
    void UseDeviceCostFunction(double covarianceScale = 1e4) { this->mDeviceCovarianceScale = covarianceScale; }
    /* ... or from the device's CostGreedyEndpoint (CostType "GreedyEndpoint", bit-exact) */
    void UseDeviceGreedyCostFunction(const csm_greedy_params& params)
    {
        this->mGreedy = params;
        this->mUseDeviceGreedy = true;
        this->mDeviceCovarianceScale = 0.0;
    }
    /* OptimizePose under a motion prior (csm_correlative_match_prior; beyond the reference): information =
     * the symmetric 3 x 3 information matrix, row-major (x, y, theta), of the sensor pose's offset from the
     * initial guess, in score units per m^2 / m rad / rad^2 (csm_host_prior_from_robot_information turns
     * one of the robot pose into it). nullptr switches the prior off. */
    void UseMotionPrior(const double information[9])
    {
        this->mUsePrior = information != nullptr;
        this->mPrior = csm_motion_prior {};
        this->mLastPrior = csm_prior_result {};
        for (int c = 0; information && c < 9; ++c)
            this->mPrior.information[c] = information[c];
    }
    /* OptimizePose on the map's likelihood field (csm_build_likelihood_map; beyond the reference, which
     * scores against the raw occupancy grid): every obstacle (value >= occupiedMin) spread by a Gaussian of
     * the sensor noise sigma, in metres, over ceil(3 sigma / resolution) cells (at most
     * CSM_LIKELIHOOD_MAX_RADIUS), so that a guess a few cells off a thin wall still scores. The field is
     * built on the device under the map's id | GridMapView::kLikelihoodIdBit, when the map is uploaded or
     * revised and on first use, and only the search reads it: the cost function, the covariance and the
     * motion prior's summary poses come from the occupancy map as before. sigma <= 0 switches it off. */
    void UseLikelihoodField(double sigma, std::uint32_t occupiedMin = 32768, bool keepUnknown = false)
    {
        CSM_ASSERT_THAT(!(sigma > 0.0 && this->mDistanceSigma > 0.0), "a likelihood field or a distance field, not both");
        this->mLikelihoodSigma = sigma;
        this->mFieldOccupiedMin = occupiedMin;
        this->mFieldKeepUnknown = keepUnknown;
        this->mFieldRevisions.clear();
    }
    /* OptimizePose on the map's distance field (csm_build_distance_map; beyond the reference): every cell
     * scores a Gaussian, of the sensor noise sigma in metres, of its distance to the NEAREST obstacle (value
     * >= occupiedMin) out to `radius` cells, 1..CSM_DISTANCE_MAX_RADIUS (0: ceil(3 sigma / resolution),
     * clamped), and 1 beyond: a slope over metres where the likelihood field ends at 16 cells. Built under
     * GridMapView::FieldId(map id, kDistanceIdBit) and kept on the terms of UseLikelihoodField; the two
     * exclude each other. sigma <= 0 switches it off. */
    void UseDistanceField(double sigma, int radius = 0, std::uint32_t occupiedMin = 32768, bool keepUnknown = false)
    {
        CSM_ASSERT_THAT(!(sigma > 0.0 && this->mLikelihoodSigma > 0.0), "a likelihood field or a distance field, not both");
        this->mDistanceSigma = sigma;
        this->mDistanceRadius = radius;
        this->mFieldOccupiedMin = occupiedMin;
        this->mFieldKeepUnknown = keepUnknown;
        this->mFieldRevisions.clear();
    }
    /* Both winners of the last OptimizePose under a prior: `unweighted` is what OptimizePose returns
     * without one, `penalty` what the prior charged the winner (key units). */
    const csm_prior_result& LastPriorResult() const { return this->mLastPrior; }

private:
    ScanMatcherCorrelativeHIP(const std::string& name, int lowResolution, double rangeX,
                              double rangeY, double rangeTheta, CostCallback costFunc,
                              detail::CtxPtr ctx) :
        mName(name), mLowResolution(lowResolution), mRangeX(rangeX), mRangeY(rangeY),
        mRangeTheta(rangeTheta), mCostFunc(costFunc), mCtx(std::move(ctx)),
        mMaps(mCtx.get(), GridMapView::kReservedIds) { }

    /* what the OptimizePose* entries share ahead of their search call: the query's map on the device for the
     * length of the call, the query as the C entries take it (on that map) and the search settings */
    struct Search {
        detail::ResidentQueryMaps::Use mMap;
        csm_loop_query mQuery;
        csm_correlative_params mParams;
    };
    Search Prepare(const ScanMatchingQuery& q, double normalizedScoreThreshold, double knownRateThreshold)
    {
        detail::ResidentQueryMaps::Use map = this->mMaps.Acquire(q.mGridMap);
        const csm_loop_query f = detail::ToLoopQuery(map.Id(), q.mGridMap, q.mScanData, q.mMapLocalInitialPose);
        return Search { std::move(map), f,
                        detail::CorrelativeParams(this->mRangeX, this->mRangeY, this->mRangeTheta, this->mLowResolution,
                                                  normalizedScoreThreshold, knownRateThreshold) };
    }

    /* The field of the resident map (the likelihood field under its id | kLikelihoodIdBit, or the distance
     * field under FieldId(id, kDistanceIdBit)): built when there is none or when it was built from another
     * revision of the map (a throw-away map: always, and released with it). */
    std::uint64_t MakeField(const GridMapView& g, detail::ResidentQueryMaps::Use& map)
    {
        csm_ctx* ctx = this->mCtx.get();
        const std::uint64_t id = map.Id();
        const bool distance = this->mDistanceSigma > 0.0;
        const std::uint64_t fieldId =
            distance ? GridMapView::FieldId(id, GridMapView::kDistanceIdBit) : id | GridMapView::kLikelihoodIdBit;
        auto held = this->mFieldRevisions.find(id);
        if (map.Temporary() || !csm_has_grid(ctx, fieldId) || held == this->mFieldRevisions.end() ||
            held->second != g.mRevision) {
            if (distance)
                this->BuildDistanceField(g, id, fieldId);
            else
                this->BuildLikelihoodField(g, id, fieldId);
            this->mFieldRevisions[id] = g.mRevision;
        }
        map.ReleaseWithIt(fieldId);
        return fieldId;
    }

    void BuildLikelihoodField(const GridMapView& g, std::uint64_t id, std::uint64_t fieldId)
    {
        csm_ctx* ctx = this->mCtx.get();
        const int radius = csm_host_likelihood_radius(this->mLikelihoodSigma, g.mResolution);
        CSM_ASSERT_THAT(radius >= 1, "likelihood sigma and map resolution > 0");
        std::vector<std::uint32_t> table(static_cast<std::size_t>(radius * radius + 1));
        CSM_ASSERT_OK(ctx, csm_host_likelihood_kernel(this->mLikelihoodSigma, g.mResolution, radius, table.data()));
        csm_likelihood_params lp {};
        lp.radius = radius;
        lp.occupied_min = this->mFieldOccupiedMin;
        lp.keep_unknown = this->mFieldKeepUnknown ? 1 : 0;
        lp.kernel = table.data();
        CSM_ASSERT_OK(ctx, csm_build_likelihood_map(ctx, id, fieldId, &lp));
    }

    void BuildDistanceField(const GridMapView& g, std::uint64_t id, std::uint64_t fieldId)
    {
        csm_ctx* ctx = this->mCtx.get();
        CSM_ASSERT_THAT(g.mResolution > 0.0, "map resolution > 0");
        int radius = this->mDistanceRadius;
        if (radius <= 0) {
            const double r = std::ceil(3.0 * (this->mDistanceSigma / g.mResolution));
            radius = r < 1.0 ? 1 : r > CSM_DISTANCE_MAX_RADIUS ? CSM_DISTANCE_MAX_RADIUS : static_cast<int>(r);
        }
        CSM_ASSERT_THAT(radius <= CSM_DISTANCE_MAX_RADIUS, "distance field radius at most %d", CSM_DISTANCE_MAX_RADIUS);
        std::vector<std::uint16_t> table(static_cast<std::size_t>(radius * radius + 1));
        CSM_ASSERT_OK(ctx, csm_host_distance_kernel(this->mDistanceSigma, g.mResolution, radius, 65534, 1, table.data()));
        csm_distance_params dp {};
        dp.radius = radius;
        dp.occupied_min = this->mFieldOccupiedMin;
        dp.keep_unknown = this->mFieldKeepUnknown ? 1 : 0;
        dp.table = table.data();
        CSM_ASSERT_OK(ctx, csm_build_distance_map(ctx, id, fieldId, &dp));
    }

    const std::string mName;
    const int mLowResolution;
    const double mRangeX, mRangeY, mRangeTheta;
    const CostCallback mCostFunc;
    detail::CtxPtr mCtx;
    detail::ResidentQueryMaps mMaps;
    double mDeviceCovarianceScale = 0.0;
    bool mUseDeviceGreedy = false;
    csm_greedy_params mGreedy {};
    bool mUsePrior = false;
    csm_motion_prior mPrior {};
    csm_prior_result mLastPrior {};
    double mLikelihoodSigma = 0.0;
    double mDistanceSigma = 0.0;
    int mDistanceRadius = 0;
    std::uint32_t mFieldOccupiedMin = 32768;       /* of the field in use, of either kind */
    bool mFieldKeepUnknown = false;
    detail::RevisionMap mFieldRevisions;       /* the map revision each resident field was built from */
};

/* ScanMatcherGridSearch (inc/mapping/scan_matcher_grid_search.hpp,
 * src/mapping/scan_matcher_grid_search.cpp:69-190): the brute-force matcher of
 * LoopDetectorGridSearch; the pixel-accurate score function is the device
 * kernel, the cost / covariance hook stays with the caller. */
class ScanMatcherGridSearchHIP final {
public:
    static std::unique_ptr<ScanMatcherGridSearchHIP> Create(
        const std::string& scanMatcherName, double rangeX, double rangeY, double rangeTheta,
        double stepX, double stepY, double stepTheta, CostCallback costFunc = nullptr,
        int deviceId = 0)
    {
        if (!(stepX > 0.0) || !(stepY > 0.0) || !(stepTheta > 0.0))
            return nullptr;
        detail::CtxPtr ctx = detail::MakeContext(deviceId);
        if (!ctx)
            return nullptr;
        return std::unique_ptr<ScanMatcherGridSearchHIP>(new ScanMatcherGridSearchHIP(
            scanMatcherName, rangeX, rangeY, rangeTheta, stepX, stepY, stepTheta, costFunc,
            std::move(ctx)));
    }

    const std::string& Name() const { return this->mName; }

    /* scan_matcher_grid_search.cpp:69-81 */
    ScanMatchingSummary OptimizePose(const ScanMatchingQuery& queryInfo)
    {
        return this->OptimizePose(queryInfo, 0.0, 0.0);
    }

    /* scan_matcher_grid_search.cpp:84-190 */
    ScanMatchingSummary OptimizePose(const ScanMatchingQuery& q,
                                     const double normalizedScoreThreshold,
                                     const double knownRateThreshold)
    {
        csm_ctx* ctx = this->mCtx.get();
        const detail::ResidentQueryMaps::Use map = this->mMaps.Acquire(q.mGridMap);
        const csm_loop_query f = detail::ToLoopQuery(map.Id(), q.mGridMap, q.mScanData, q.mMapLocalInitialPose);
        const csm_grid_search_params prm { this->mRangeX, this->mRangeY, this->mRangeTheta,
                                           this->mStepX, this->mStepY, this->mStepTheta,
                                           normalizedScoreThreshold, knownRateThreshold };
        csm_summary s {};
        CSM_ASSERT_OK(ctx, csm_grid_search_match(ctx, f.map_id, &f.geometry, &f.scan, f.initial_pose, &prm, &s));
        ScanMatchingSummary out;
        detail::FillSummary(s, q.mMapLocalInitialPose, &out);
        if (this->mCostFunc)
            this->mCostFunc(q, out.mBestSensorPose, &out.mNormalizedCost, out.mEstimatedCovariance);
        else if (this->mUseDeviceGreedy)
            detail::DeviceGreedyCost(ctx, f, s.best_sensor_pose, this->mGreedy, &out);
        return out;
    }

    /* Cost and covariance from the device's CostGreedyEndpoint (the default cost of
     * LoopDetectorGridSearch, launcher_settings_default.json:80) instead of a host callback */
    void UseDeviceGreedyCostFunction(const csm_greedy_params& params)
    {
        this->mGreedy = params;
        this->mUseDeviceGreedy = true;
    }

private:
    ScanMatcherGridSearchHIP(const std::string& name, double rangeX, double rangeY,
                             double rangeTheta, double stepX, double stepY, double stepTheta,
                             CostCallback costFunc, detail::CtxPtr ctx) :
        mName(name), mRangeX(rangeX), mRangeY(rangeY), mRangeTheta(rangeTheta), mStepX(stepX),
        mStepY(stepY), mStepTheta(stepTheta), mCostFunc(costFunc), mCtx(std::move(ctx)),
        mMaps(mCtx.get(), GridMapView::kReservedIds + 1) { }

    const std::string mName;
    const double mRangeX, mRangeY, mRangeTheta;
    const double mStepX, mStepY, mStepTheta;
    const CostCallback mCostFunc;
    detail::CtxPtr mCtx;
    detail::ResidentQueryMaps mMaps;
    bool mUseDeviceGreedy = false;
    csm_greedy_params mGreedy {};
};

/* ScanMatcherHillClimbing with the GreedyEndpoint cost
 * (inc/mapping/scan_matcher_hill_climbing.hpp, src/mapping/scan_matcher_hill_climbing.cpp:72-180;
 * factory src/scan_matcher_factory.cpp:103-130): the whole search, the cost and the covariance on
 * the device, bit-exact. LastResult() holds the metric inputs of the last call (NumOfIterations,
 * NumOfRefinements, InitialCost, FinalCost, DiffTranslation, DiffRotation). */
class ScanMatcherHillClimbingHIP final {
public:
    static std::unique_ptr<ScanMatcherHillClimbingHIP> Create(
        const std::string& scanMatcherName, double linearStep, double angularStep, int maxIterations,
        int maxNumOfRefinements, const csm_greedy_params& costParams, int deviceId = 0)
    {
        if (!(linearStep > 0.0) || !(angularStep > 0.0) || maxIterations < 1)
            return nullptr;
        detail::CtxPtr ctx = detail::MakeContext(deviceId);
        if (!ctx)
            return nullptr;
        csm_hill_climbing_params prm {};
        prm.linear_step = linearStep;
        prm.angular_step = angularStep;
        prm.max_iterations = maxIterations;
        prm.max_refinements = maxNumOfRefinements;
        prm.cost = costParams;
        return std::unique_ptr<ScanMatcherHillClimbingHIP>(
            new ScanMatcherHillClimbingHIP(scanMatcherName, prm, std::move(ctx)));
    }

    ScanMatcherHillClimbingHIP(const ScanMatcherHillClimbingHIP&) = delete;
    ScanMatcherHillClimbingHIP& operator=(const ScanMatcherHillClimbingHIP&) = delete;

    const std::string& Name() const { return this->mName; }
    csm_ctx* Context() const { return this->mCtx.get(); }
    const csm_hill_climbing_result& LastResult() const { return this->mLast; }

    ScanMatchingSummary OptimizePose(const ScanMatchingQuery& q)
    {
        csm_ctx* ctx = this->mCtx.get();
        const detail::ResidentQueryMaps::Use map = this->mMaps.Acquire(q.mGridMap);
        const csm_loop_query f = detail::ToLoopQuery(map.Id(), q.mGridMap, q.mScanData, q.mMapLocalInitialPose);
        CSM_ASSERT_OK(ctx, csm_hill_climbing_batch(ctx, &f, 1, &this->mParams, &this->mLast));
        const csm_hill_climbing_result& r = this->mLast;
        ScanMatchingSummary out;
        out.mPoseFound = true;      /* scan_matcher_hill_climbing.cpp:176-179 */
        out.mNormalizedCost = r.normalized_cost;
        out.mMapLocalInitialPose = q.mMapLocalInitialPose;
        out.mEstimatedPose = { r.estimated_pose[0], r.estimated_pose[1], r.estimated_pose[2] };
        out.mBestSensorPose = { r.best_sensor_pose[0], r.best_sensor_pose[1], r.best_sensor_pose[2] };
        for (int c = 0; c < 9; ++c)
            out.mEstimatedCovariance[c] = r.covariance[c];
        out.mNumOfCandidates = r.cost_evaluations;
        return out;
    }

private:
    ScanMatcherHillClimbingHIP(const std::string& name, const csm_hill_climbing_params& prm,
                               detail::CtxPtr ctx) :
        mName(name), mParams(prm), mCtx(std::move(ctx)), mMaps(mCtx.get(), GridMapView::kReservedIds + 2) { }

    const std::string mName;
    const csm_hill_climbing_params mParams;
    detail::CtxPtr mCtx;
    detail::ResidentQueryMaps mMaps;
    csm_hill_climbing_result mLast {};
};

/* inc/mapping/loop_detector.hpp:27-55, flattened to what the search reads:
 * the reference local map (finished, immutable, keyed by LocalMapId) and the
 * query scan node's scan + its pose local to that map
 * (InverseCompound(localMapNode.mGlobalPose, scanNode.mGlobalPose),
 * loop_detector_branch_bound.cpp:97-98 -- the caller passes both global poses). */
struct LoopDetectionQuery {
    GridMapView mReferenceLocalMap;
    ScanDataView mQueryScanData;
    RobotPose2D<double> mQueryScanNodeGlobalPose;
    RobotPose2D<double> mReferenceLocalMapNodeGlobalPose;
    int mQueryScanNodeId = 0;
};
using LoopDetectionQueryVector = std::vector<LoopDetectionQuery>;

/* inc/mapping/loop_detector.hpp:58-92. Without a final matcher
 * (UseFinalScanMatcher) mRelativePose is the search's estimate and the
 * covariance is zero; with one they are ScanMatcherLinearSolver's
 * (loop_detector_branch_bound.cpp:123-135). */
struct LoopDetectionResult {
    RobotPose2D<double> mRelativePose;   /* estimated pose, map-local */
    RobotPose2D<double> mLocalMapPose;
    std::uint64_t mLocalMapNodeId;
    int mScanNodeId;
    double mScoreValue;
    std::uint32_t mFlags;
    double mEstimatedCovariance[9] = { 0 };   /* row-major */
    double mNormalizedCost = 0.0;
};
using LoopDetectionResultVector = std::vector<LoopDetectionResult>;

/* The free-space check of loop candidates (csm_ray_check_batch, include/csm_hip.h): every beam of the query
 * scan walked from the sensor to its hit at the candidate pose, the cells it crosses classified against the
 * reference local map. A correlative score only counts where the end points fall; a pose on the wrong side
 * of a wall scores like the true one, and only its rays run through cells the map knows to be occupied.
 * A candidate is kept iff all three hold:
 *   walked >= mMinWalked,  blocked <= mMaxBlockedRate * walked,  end_occupied >= mMinEndOccupiedRate * end_inside */
struct RayCheckSettings {
    csm_ray_check_params mParams {};
    double mMaxBlockedRate = 0.1;
    int mMinWalked = 1;
    double mMinEndOccupiedRate = 0.0;

    /* the builder's usable range and sub-pixel scale; occupied / free at P >= probOccupied / P <= probFree */
    static RayCheckSettings Create(double usableRangeMin = 0.01, double usableRangeMax = 20.0,
                                   double probOccupied = 0.65, double probFree = 0.35, int endTolerance = 1,
                                   int subpixelScale = 100)
    {
        RayCheckSettings s;
        s.mParams.usable_range_min = usableRangeMin;
        s.mParams.usable_range_max = usableRangeMax;
        s.mParams.subpixel_scale = subpixelScale;
        s.mParams.end_tolerance = endTolerance;
        CSM_ASSERT_OK(nullptr, csm_host_ray_check_values(probOccupied, probFree, &s.mParams.occupied_min,
                                                         &s.mParams.free_max));
        return s;
    }

    bool Passes(const csm_ray_check_result& r) const
    {
        return r.walked >= this->mMinWalked &&
               static_cast<double>(r.blocked) <= this->mMaxBlockedRate * static_cast<double>(r.walked) &&
               static_cast<double>(r.end_occupied) >= this->mMinEndOccupiedRate * static_cast<double>(r.end_inside);
    }
};

/* DetectChecked / DetectPeaksChecked: the results that pass, each with its record beside it, and every
 * candidate that was checked (mQueryIndex: its query; mPeakIndex: its place among the query's peaks, 0 for
 * DetectChecked; mKept) with its record, so that a caller can see why one was dropped. */
struct CheckedLoopDetections {
    LoopDetectionResultVector mResults;
    std::vector<csm_ray_check_result> mRecords;              /* beside mResults */
    LoopDetectionResultVector mCandidates;
    std::vector<csm_ray_check_result> mCandidateRecords;     /* beside mCandidates */
    std::vector<int> mQueryIndex, mPeakIndex;
    std::vector<char> mKept;
};

namespace detail {
/* A reference local map is uploaded once per id and context (mPrecompMaps, loop_detector_branch_bound.hpp:98):
 * a loop detector only sees finished local maps, which have an id and never change
 * (Assert(localMap.mFinished), loop_detector_branch_bound.cpp:77) */
inline void UploadOnce(csm_ctx* ctx, const GridMapView& g)
{
    CSM_ASSERT_THAT(g.mId != GridMapView::kInvalidId, "reference local map without an id");
    if (!csm_has_grid(ctx, g.mId))
        CSM_ASSERT_OK(ctx, csm_upload_grid(ctx, g.mId, g.mValues, g.mRows, g.mCols));
}

/* query q at the map-local robot pose `pose` */
inline csm_loop_query ToLoopQuery(const LoopDetectionQuery& q, const RobotPose2D<double>& pose)
{
    return ToLoopQuery(q.mReferenceLocalMap.mId, q.mReferenceLocalMap, q.mQueryScanData, pose);
}

/* query q at its initial pose, InverseCompound(localMapNode.mGlobalPose, scanNode.mGlobalPose) */
inline csm_loop_query ToLoopQuery(const LoopDetectionQuery& q)
{
    csm_loop_query f = ToLoopQuery(q, RobotPose2D<double> { 0.0, 0.0, 0.0 });
    const double start[3] = { q.mReferenceLocalMapNodeGlobalPose.mX, q.mReferenceLocalMapNodeGlobalPose.mY,
                              q.mReferenceLocalMapNodeGlobalPose.mTheta };
    const double end[3] = { q.mQueryScanNodeGlobalPose.mX, q.mQueryScanNodeGlobalPose.mY,
                            q.mQueryScanNodeGlobalPose.mTheta };
    csm_host_inverse_compound(start, end, f.initial_pose);
    return f;
}

inline LoopDetectionResult ToResult(const LoopDetectionQuery& q, const csm_summary& s)
{
    return LoopDetectionResult { { s.estimated_pose[0], s.estimated_pose[1], s.estimated_pose[2] },
                                 q.mReferenceLocalMapNodeGlobalPose, q.mReferenceLocalMap.mId,
                                 q.mQueryScanNodeId, s.raw.score, s.raw.flags };
}

/* the candidates of a DetectFound(): candidate j belongs to query found[j] and is its only peak */
inline void SetCandidates(LoopDetectionResultVector candidates, const std::vector<std::size_t>& found,
                          CheckedLoopDetections& checked)
{
    checked.mCandidates = std::move(candidates);
    for (std::size_t i : found) {
        checked.mQueryIndex.push_back(static_cast<int>(i));
        checked.mPeakIndex.push_back(0);
    }
}

/* the map-local robot poses at which the candidates are checked */
inline std::vector<RobotPose2D<double>> CandidatePoses(const CheckedLoopDetections& checked)
{
    std::vector<RobotPose2D<double>> poses;
    for (const LoopDetectionResult& r : checked.mCandidates)
        poses.push_back(r.mRelativePose);
    return poses;
}

/* mKept[j] = settings.Passes(mCandidateRecords[j]) */
inline void MarkKept(const RayCheckSettings& settings, CheckedLoopDetections& checked)
{
    checked.mKept.clear();
    for (const csm_ray_check_result& r : checked.mCandidateRecords)
        checked.mKept.push_back(settings.Passes(r) ? 1 : 0);
}

/* mResults / mRecords = the kept candidates. firstPerQuery: of a query's candidates (its peaks, best first)
 * only the first kept one stays kept; the mark of every later one is taken back. */
inline void CollectKept(CheckedLoopDetections& checked, bool firstPerQuery)
{
    int taken = -1;                     /* the last query that has its peak */
    for (std::size_t j = 0; j < checked.mCandidates.size(); ++j) {
        if (checked.mKept[j] && !(firstPerQuery && checked.mQueryIndex[j] == taken)) {
            taken = checked.mQueryIndex[j];
            checked.mResults.push_back(checked.mCandidates[j]);
            checked.mRecords.push_back(checked.mCandidateRecords[j]);
        } else {
            checked.mKept[j] = 0;
        }
    }
}
} /* namespace detail */

class LoopDetectorBranchBoundHIP final {
public:
    /* scoreThreshold / knownRateThreshold as LoopDetectorBranchBound
     * (src/mapping/loop_detector_branch_bound.cpp:38-56); nodeHeightMax and the
     * search ranges as its ScanMatcherBranchBound
     * (src/scan_matcher_factory.cpp:22-26). deviceIds: the GPUs the detector
     * spreads a Detect() call over -- contiguous blocks of the query vector, one
     * host thread per GPU inside the library, as LoopDetectorFPGAParallel does
     * with its two FPGA cores (src/mapping/loop_detector_fpga_parallel.cpp:42-56). */
    static std::unique_ptr<LoopDetectorBranchBoundHIP> Create(
        const std::string& loopDetectorName, int nodeHeightMax, double rangeX, double rangeY,
        double rangeTheta, double scoreThreshold, double knownRateThreshold,
        const std::vector<int>& deviceIds)
    {
        if (!(scoreThreshold > 0.0 && scoreThreshold <= 1.0) ||
            !(knownRateThreshold > 0.0 && knownRateThreshold <= 1.0) || deviceIds.empty())
            return nullptr;
        std::vector<std::int32_t> ids(deviceIds.begin(), deviceIds.end());
        csm_group* group = nullptr;
        if (csm_group_create(ids.data(), static_cast<std::int32_t>(ids.size()), &group) != 0)
            return nullptr;
        return std::unique_ptr<LoopDetectorBranchBoundHIP>(new LoopDetectorBranchBoundHIP(
            loopDetectorName, nodeHeightMax, rangeX, rangeY, rangeTheta, scoreThreshold,
            knownRateThreshold, group));
    }

    static std::unique_ptr<LoopDetectorBranchBoundHIP> Create(
        const std::string& loopDetectorName, int nodeHeightMax, double rangeX, double rangeY,
        double rangeTheta, double scoreThreshold, double knownRateThreshold, int deviceId = 0)
    {
        return Create(loopDetectorName, nodeHeightMax, rangeX, rangeY, rangeTheta, scoreThreshold,
                      knownRateThreshold, std::vector<int> { deviceId });
    }

    ~LoopDetectorBranchBoundHIP() { csm_group_destroy(this->mGroup); }
    LoopDetectorBranchBoundHIP(const LoopDetectorBranchBoundHIP&) = delete;
    LoopDetectorBranchBoundHIP& operator=(const LoopDetectorBranchBoundHIP&) = delete;

    const std::string& Name() const { return this->mName; }
    int NumOfDevices() const { return csm_group_size(this->mGroup); }

    /* The detector's final matcher, ScanMatcherLinearSolver on CostSquareError
     * ("FinalScanMatcherLinearSolver", launcher_settings_default.json:148-155, 11-13),
     * run on the device for all found queries of a Detect() call. */
    void UseFinalScanMatcher(int numOfIterationsMax = 10, double convergenceThreshold = 1e-4,
                             double initialLambda = 1e-4, double covarianceScale = 1e4)
    {
        this->mRefine = true;
        this->mRefineParams.iterations_max = numOfIterationsMax;
        this->mRefineParams.convergence_threshold = convergenceThreshold;
        this->mRefineParams.lambda = initialLambda;
        this->mRefineParams.covariance_scale = covarianceScale;
    }

    /* LoopDetector::Detect: results only for the queries where a pose was
     * found, in query order (loop_detector_branch_bound.cpp:107-135). */
    LoopDetectionResultVector Detect(const LoopDetectionQueryVector& queries)
    {
        return this->DetectFound(queries, nullptr);
    }

    /* The free-space check of queries[i]'s scan at poses[i] (map-local robot poses) against its reference
     * local map, each member of the group on its block of the queries: one record per query. */
    std::vector<csm_ray_check_result> CheckRays(const LoopDetectionQueryVector& queries,
                                                const std::vector<RobotPose2D<double>>& poses,
                                                const RayCheckSettings& settings)
    {
        CSM_ASSERT_THAT(queries.empty() || poses.size() == queries.size(), "one pose per query");
        std::vector<int> all(queries.size());
        std::iota(all.begin(), all.end(), 0);
        return this->CheckAt(queries, all, poses, settings);
    }

    /* Detect(), then one free-space check per member over the found queries at their result poses: a result
     * is kept iff settings.Passes(its record). */
    CheckedLoopDetections DetectChecked(const LoopDetectionQueryVector& queries, const RayCheckSettings& settings)
    {
        CheckedLoopDetections checked;
        std::vector<std::size_t> found;
        detail::SetCandidates(this->DetectFound(queries, &found), found, checked);
        checked.mCandidateRecords = this->CheckAt(queries, checked.mQueryIndex, detail::CandidatePoses(checked), settings);
        detail::MarkKept(settings, checked);
        detail::CollectKept(checked, false);
        return checked;
    }

private:
    /* fn(ctx, at) for every member that has work: ctx is the member's context and `at` the places j of
     * `index` whose query index[j] lies in the member's block. The blocks are those of the whole query vector
     * (numOfQueries), whatever `index` selects: each member holds the maps of its own block, so that what
     * follows a Detect() runs where Detect() ran. */
    template <typename Fn>
    void ForEachMember(std::size_t numOfQueries, const std::vector<int>& index, Fn&& fn) const
    {
        const std::int32_t members = csm_group_size(this->mGroup);
        for (std::int32_t k = 0; k < members; ++k) {
            std::int32_t lo = 0, hi = 0;
            csm_shard_bounds(static_cast<std::int32_t>(numOfQueries), k, members, &lo, &hi);
            std::vector<std::size_t> at;
            for (std::size_t j = 0; j < index.size(); ++j)
                if (index[j] >= lo && index[j] < hi)
                    at.push_back(j);
            if (!at.empty())
                fn(csm_group_member(this->mGroup, k), at);
        }
    }

    /* record j = the free-space check of queries[index[j]]'s scan at poses[j], each member on its block */
    std::vector<csm_ray_check_result> CheckAt(const LoopDetectionQueryVector& queries, const std::vector<int>& index,
                                              const std::vector<RobotPose2D<double>>& poses,
                                              const RayCheckSettings& settings) const
    {
        std::vector<csm_ray_check_result> records(index.size());
        this->ForEachMember(queries.size(), index, [&](csm_ctx* ctx, const std::vector<std::size_t>& at) {
            std::vector<csm_loop_query> flat;
            for (std::size_t j : at) {
                const LoopDetectionQuery& q = queries[static_cast<std::size_t>(index[j])];
                detail::UploadOnce(ctx, q.mReferenceLocalMap);
                flat.push_back(detail::ToLoopQuery(q, poses[j]));
            }
            std::vector<csm_ray_check_result> res(flat.size());
            CSM_ASSERT_OK(ctx, csm_ray_check_batch(ctx, flat.data(), static_cast<std::int32_t>(flat.size()),
                                                   &settings.mParams, res.data(), nullptr));
            for (std::size_t j = 0; j < at.size(); ++j)
                records[at[j]] = res[j];
        });
        return records;
    }

    /* Detect(); found (may be null) receives the query index of every result */
    LoopDetectionResultVector DetectFound(const LoopDetectionQueryVector& queries, std::vector<std::size_t>* found)
    {
        LoopDetectionResultVector results;
        if (queries.empty())
            return results;
        std::vector<csm_loop_query> flat(queries.size());
        std::vector<int> all(queries.size());
        std::iota(all.begin(), all.end(), 0);
        this->ForEachMember(queries.size(), all, [&](csm_ctx* ctx, const std::vector<std::size_t>& at) {
            for (std::size_t i : at) {
                detail::UploadOnce(ctx, queries[i].mReferenceLocalMap);
                flat[i] = detail::ToLoopQuery(queries[i]);
            }
        });
        csm_bnb_params prm {};
        prm.range_x = this->mRangeX;
        prm.range_y = this->mRangeY;
        prm.range_theta = this->mRangeTheta;
        prm.node_height_max = this->mNodeHeightMax;
        prm.score_threshold = this->mScoreThreshold;
        prm.known_rate_threshold = this->mKnownRateThreshold;
        std::vector<csm_summary> out(queries.size());
        const int rc = csm_group_bnb_match_batch(this->mGroup, flat.data(), static_cast<std::int32_t>(flat.size()), &prm,
                                                 out.data());
        CSM_ASSERT_THAT(rc == 0, "csm_group_bnb_match_batch == 0 (rc %d: %s)", rc, csm_group_last_error(this->mGroup));
        std::vector<int> hits;              /* the queries where a pose was found */
        for (std::size_t i = 0; i < queries.size(); ++i)
            if (out[i].pose_found) {
                results.push_back(detail::ToResult(queries[i], out[i]));
                hits.push_back(static_cast<int>(i));
                if (found)
                    found->push_back(i);
            }
        if (!this->mRefine)
            return results;
        /* the final matcher on every estimate that was found, member by member:
         * loop_detector_branch_bound.cpp:119-127 */
        this->ForEachMember(queries.size(), hits, [&](csm_ctx* ctx, const std::vector<std::size_t>& at) {
            std::vector<csm_loop_query> second;
            for (std::size_t j : at) {
                second.push_back(flat[static_cast<std::size_t>(hits[j])]);
                for (int c = 0; c < 3; ++c)
                    second.back().initial_pose[c] = out[static_cast<std::size_t>(hits[j])].estimated_pose[c];
            }
            std::vector<csm_refine_result> res(second.size());
            CSM_ASSERT_OK(ctx, csm_linear_solver_batch(ctx, second.data(), static_cast<std::int32_t>(second.size()),
                                                       &this->mRefineParams, res.data()));
            for (std::size_t j = 0; j < at.size(); ++j) {
                LoopDetectionResult& r = results[at[j]];
                r.mRelativePose = { res[j].estimated_pose[0], res[j].estimated_pose[1], res[j].estimated_pose[2] };
                for (int c = 0; c < 9; ++c)
                    r.mEstimatedCovariance[c] = res[j].covariance[c];
                r.mNormalizedCost = res[j].normalized_cost;
            }
            /* the solver object keeps its damping factor between calls */
            this->mRefineParams.lambda = res.back().lambda;
        });
        return results;
    }

    LoopDetectorBranchBoundHIP(const std::string& name, int nodeHeightMax, double rangeX,
                               double rangeY, double rangeTheta, double scoreThreshold,
                               double knownRateThreshold, csm_group* group) :
        mName(name), mNodeHeightMax(nodeHeightMax), mRangeX(rangeX), mRangeY(rangeY),
        mRangeTheta(rangeTheta), mScoreThreshold(scoreThreshold),
        mKnownRateThreshold(knownRateThreshold), mGroup(group) { }

    const std::string mName;
    const int mNodeHeightMax;
    const double mRangeX, mRangeY, mRangeTheta;
    const double mScoreThreshold, mKnownRateThreshold;
    csm_group* mGroup;
    bool mRefine = false;
    csm_refine_params mRefineParams {};
};

/* LoopDetectorCorrelative (the reference's default "RealTimeCorrelative" loop
 * detector, launcher_settings_default.json:101-114, 394): the correlative
 * matcher with the detector's thresholds, one coarse map cached per local map. */
class LoopDetectorCorrelativeHIP final {
public:
    static std::unique_ptr<LoopDetectorCorrelativeHIP> Create(
        const std::string& loopDetectorName, int lowResolution, double rangeX, double rangeY,
        double rangeTheta, double scoreThreshold, double knownRateThreshold, int deviceId = 0)
    {
        /* src/mapping/loop_detector_correlative.cpp:38-56 */
        if (!(scoreThreshold > 0.0 && scoreThreshold <= 1.0) ||
            !(knownRateThreshold > 0.0 && knownRateThreshold <= 1.0) || lowResolution < 1)
            return nullptr;
        detail::CtxPtr ctx = detail::MakeContext(deviceId);
        if (!ctx)
            return nullptr;
        return std::unique_ptr<LoopDetectorCorrelativeHIP>(new LoopDetectorCorrelativeHIP(
            loopDetectorName, lowResolution, rangeX, rangeY, rangeTheta, scoreThreshold,
            knownRateThreshold, std::move(ctx)));
    }

    const std::string& Name() const { return this->mName; }

    LoopDetectionResultVector Detect(const LoopDetectionQueryVector& queries)
    {
        return this->DetectFound(queries, nullptr);
    }

    /* The free-space check of queries[i]'s scan at poses[i] (map-local robot poses) against its reference
     * local map, all queries in one csm_ray_check_batch: one record per query. */
    std::vector<csm_ray_check_result> CheckRays(const LoopDetectionQueryVector& queries,
                                                const std::vector<RobotPose2D<double>>& poses,
                                                const RayCheckSettings& settings)
    {
        std::vector<csm_ray_check_result> records(queries.size());
        if (queries.empty())
            return records;
        CSM_ASSERT_THAT(poses.size() == queries.size(), "one pose per query");
        csm_ctx* ctx = this->mCtx.get();
        std::vector<csm_loop_query> flat(queries.size());
        for (std::size_t i = 0; i < queries.size(); ++i) {
            detail::UploadOnce(ctx, queries[i].mReferenceLocalMap);
            flat[i] = detail::ToLoopQuery(queries[i], poses[i]);
        }
        CSM_ASSERT_OK(ctx, csm_ray_check_batch(ctx, flat.data(), static_cast<std::int32_t>(flat.size()),
                                               &settings.mParams, records.data(), nullptr));
        return records;
    }

    /* Detect(), then one csm_ray_check_batch over the found queries at their estimated poses: a result is
     * kept iff settings.Passes(its record). */
    CheckedLoopDetections DetectChecked(const LoopDetectionQueryVector& queries, const RayCheckSettings& settings)
    {
        CheckedLoopDetections checked;
        std::vector<std::size_t> found;
        detail::SetCandidates(this->DetectFound(queries, &found), found, checked);
        this->CheckCandidates(queries, settings, checked, false);
        return checked;
    }

    /* DetectPeaks(), then ALL peaks of ALL queries in one csm_ray_check_batch; per query the first peak
     * (best first) that passes is kept. mKept marks that peak alone: a later peak of the same query is not
     * kept even where its record passes. */
    CheckedLoopDetections DetectPeaksChecked(const LoopDetectionQueryVector& queries, int numOfPeaks, int exclX,
                                             int exclY, int exclTheta, const RayCheckSettings& settings)
    {
        CheckedLoopDetections checked;
        const std::vector<LoopDetectionResultVector> peaks = this->DetectPeaks(queries, numOfPeaks, exclX, exclY,
                                                                               exclTheta);
        for (std::size_t i = 0; i < peaks.size(); ++i)
            for (std::size_t j = 0; j < peaks[i].size(); ++j) {
                checked.mCandidates.push_back(peaks[i][j]);
                checked.mQueryIndex.push_back(static_cast<int>(i));
                checked.mPeakIndex.push_back(static_cast<int>(j));
            }
        this->CheckCandidates(queries, settings, checked, true);
        return checked;
    }

    /* Detect() keeping up to numOfPeaks DISTINCT poses per query, best first
     * (csm_correlative_peaks_batch): element i holds the peaks of queries[i] that pass the score
     * threshold, none when Detect() would have skipped the query. A second entry scoring close to the
     * first says the match is ambiguous (a corridor, repeated structure): the caller can drop the loop
     * edge instead of adding a wrong one. exclX / exclY / exclTheta: half-widths, in search steps, of
     * the box around a chosen pose in which no later one is taken. */
    std::vector<LoopDetectionResultVector> DetectPeaks(const LoopDetectionQueryVector& queries, int numOfPeaks,
                                                       int exclX, int exclY, int exclTheta)
    {
        std::vector<LoopDetectionResultVector> results(queries.size());
        if (queries.empty())
            return results;
        csm_ctx* ctx = this->mCtx.get();
        const std::vector<csm_loop_query> flat = this->Flatten(queries);
        const csm_correlative_params prm = this->Params();
        const csm_peaks_params peaks { numOfPeaks, exclX, exclY, exclTheta, 0 };
        const std::size_t kMax = static_cast<std::size_t>(std::max(1, std::min(numOfPeaks, CSM_PEAKS_MAX)));
        std::vector<csm_summary> out(queries.size() * kMax);
        std::vector<std::int32_t> count(queries.size(), 0);
        CSM_ASSERT_OK(ctx, csm_correlative_peaks_batch(ctx, flat.data(), static_cast<std::int32_t>(flat.size()), &prm,
                                                       &peaks, out.data(), count.data()));
        for (std::size_t i = 0; i < queries.size(); ++i)
            for (std::int32_t j = 0; j < count[i]; ++j)
                results[i].push_back(detail::ToResult(queries[i], out[i * kMax + static_cast<std::size_t>(j)]));
        return results;
    }

    /* Detect() with every result's mEstimatedCovariance read off its window's whole score volume
     * (csm_correlative_covariance_batch; see ScanMatcherCorrelativeHIP::OptimizePoseVolumeCovariance): the
     * information matrix of the loop edge then says how ambiguous the window was. *borderSupport
     * (optional) receives, per result, the weighted candidates on a face of its window. */
    LoopDetectionResultVector DetectVolumeCovariance(const LoopDetectionQueryVector& queries, double temperature,
                                                     std::vector<long long>* borderSupport = nullptr)
    {
        LoopDetectionResultVector results;
        if (borderSupport)
            borderSupport->clear();
        if (queries.empty())
            return results;
        csm_ctx* ctx = this->mCtx.get();
        const std::vector<csm_loop_query> flat = this->Flatten(queries);
        const csm_correlative_params prm = this->Params();
        const csm_volume_params volume { temperature, 0 };
        std::vector<csm_volume_summary> out(queries.size());
        CSM_ASSERT_OK(ctx, csm_correlative_covariance_batch(ctx, flat.data(), static_cast<std::int32_t>(flat.size()),
                                                            &prm, &volume, out.data()));
        for (std::size_t i = 0; i < queries.size(); ++i) {
            if (!out[i].summary.pose_found)
                continue;
            LoopDetectionResult r = detail::ToResult(queries[i], out[i].summary);
            for (int c = 0; c < 9; ++c)
                r.mEstimatedCovariance[c] = out[i].covariance[c];
            results.push_back(r);
            if (borderSupport)
                borderSupport->push_back(out[i].moments.border_support);
        }
        return results;
    }

private:
    /* Detect(); found (may be null) receives the query index of every result */
    LoopDetectionResultVector DetectFound(const LoopDetectionQueryVector& queries, std::vector<std::size_t>* found)
    {
        LoopDetectionResultVector results;
        if (queries.empty())
            return results;
        csm_ctx* ctx = this->mCtx.get();
        const std::vector<csm_loop_query> flat = this->Flatten(queries);
        const csm_correlative_params prm = this->Params();
        std::vector<csm_summary> out(queries.size());
        CSM_ASSERT_OK(ctx, csm_correlative_match_batch(
                               ctx, flat.data(), static_cast<std::int32_t>(flat.size()), &prm, out.data()));
        for (std::size_t i = 0; i < queries.size(); ++i)
            if (out[i].pose_found) {
                results.push_back(detail::ToResult(queries[i], out[i]));
                if (found)
                    found->push_back(i);
            }
        return results;
    }

    /* the records of checked.mCandidates (query mQueryIndex[j] at the candidate's pose) in one call, then
     * mKept, mResults and mRecords from them */
    void CheckCandidates(const LoopDetectionQueryVector& queries, const RayCheckSettings& settings,
                         CheckedLoopDetections& checked, bool firstPerQuery)
    {
        LoopDetectionQueryVector sub;
        for (int i : checked.mQueryIndex)
            sub.push_back(queries[static_cast<std::size_t>(i)]);
        checked.mCandidateRecords = this->CheckRays(sub, detail::CandidatePoses(checked), settings);
        detail::MarkKept(settings, checked);
        detail::CollectKept(checked, firstPerQuery);
    }

    /* the queries as the batch entries take them; maps that are not resident yet are uploaded */
    std::vector<csm_loop_query> Flatten(const LoopDetectionQueryVector& queries)
    {
        std::vector<csm_loop_query> flat(queries.size());
        for (std::size_t i = 0; i < queries.size(); ++i) {
            detail::UploadOnce(this->mCtx.get(), queries[i].mReferenceLocalMap);
            flat[i] = detail::ToLoopQuery(queries[i]);
        }
        return flat;
    }

    csm_correlative_params Params() const
    {
        return detail::CorrelativeParams(this->mRangeX, this->mRangeY, this->mRangeTheta, this->mLowResolution,
                                         this->mScoreThreshold, this->mKnownRateThreshold);
    }

    LoopDetectorCorrelativeHIP(const std::string& name, int lowResolution, double rangeX,
                               double rangeY, double rangeTheta, double scoreThreshold,
                               double knownRateThreshold, detail::CtxPtr ctx) :
        mName(name), mLowResolution(lowResolution), mRangeX(rangeX), mRangeY(rangeY),
        mRangeTheta(rangeTheta), mScoreThreshold(scoreThreshold),
        mKnownRateThreshold(knownRateThreshold), mCtx(std::move(ctx)) { }

    const std::string mName;
    const int mLowResolution;
    const double mRangeX, mRangeY, mRangeTheta;
    const double mScoreThreshold, mKnownRateThreshold;
    detail::CtxPtr mCtx;
};

/* The latest-map half of GridMapBuilder (src/mapping/grid_map_builder.cpp): the
 * map the frontend matches every new scan against is rebuilt from the last
 * mNumOfScansForLatestMap scans on every call (UpdateLatestMap, :497-527).
 * Here it is built on the device and stays there under one map id, so the
 * matcher needs no upload; pass the matcher's Context() to share it. */
class GridMapBuilderHIP final {
public:
    /* constructor arguments as GridMapBuilder (grid_map_builder.cpp:68-99) minus
     * the local-map ones; `ctx` is borrowed */
    GridMapBuilderHIP(csm_ctx* ctx, double mapResolution, int patchSize, int numOfScansForLatestMap,
                      double usableRangeMin, double usableRangeMax, double probHit,
                      double probMiss, std::uint64_t latestMapId = (1ull << 61)) :
        mCtx(ctx), mNumOfScansForLatestMap(numOfScansForLatestMap), mLatestMapPose { 0.0, 0.0, 0.0 }
    {
        this->mParams = { usableRangeMin, usableRangeMax, probHit, probMiss, 100 };   /* SubpixelScale */
        /* GridMap(resolution, patchSize, 1.0, 1.0) (grid_map.cpp:75-98, 224-246) */
        int log2Block = 0;
        while ((1 << log2Block) < patchSize)
            ++log2Block;
        const int block = 1 << log2Block;
        const int desired = static_cast<int>(std::ceil(1.0 / mapResolution));
        const int cells = ((desired + block - 1) >> log2Block) << log2Block;
        this->mShape = { mapResolution, 0.0, 0.0, cells, cells, log2Block };
        this->mInitialCells = cells;
        this->mLatestMap.mId = latestMapId;
        this->SyncView();
    }

    /* geometry + id of the latest map; mValues is null: the cells live on the device */
    const GridMapView& LatestMap() const { return this->mLatestMap; }
    const RobotPose2D<double>& LatestMapPose() const { return this->mLatestMapPose; }
    const csm_map_build_info& LastBuildInfo() const { return this->mInfo; }

    /* GridMapBuilder::UpdateLatestMap (grid_map_builder.cpp:497-527); scanNodes in id order */
    void UpdateLatestMap(const std::vector<ScanNodeView>& scanNodes)
    {
        CSM_ASSERT_THAT(!scanNodes.empty(), "!scanNodes.empty()");
        const std::size_t count = std::min(scanNodes.size(),
                                           static_cast<std::size_t>(this->mNumOfScansForLatestMap));
        const ScanNodeView* first = scanNodes.data() + (scanNodes.size() - count);
        this->mLatestMapPose = first->mGlobalPose;
        this->ConstructMapFromScans(this->mLatestMapPose, first, count);
    }

    /* GridMapBuilder::ConstructMapFromScans (grid_map_builder.cpp:561-695) into the latest map */
    void ConstructMapFromScans(const RobotPose2D<double>& globalMapPose, const ScanNodeView* nodes,
                               std::size_t numOfNodes)
    {
        const std::vector<csm_scan_node> flat = detail::ToScanNodes(nodes, numOfNodes);
        const double pose[3] = { globalMapPose.mX, globalMapPose.mY, globalMapPose.mTheta };
        CSM_ASSERT_OK(this->mCtx, csm_construct_map_from_scans(
                                      this->mCtx, this->mLatestMap.mId, &this->mShape, pose, flat.data(),
                                      static_cast<std::int32_t>(numOfNodes), &this->mParams, &this->mInfo));
        this->SyncView();
    }

    /* GridMap::CopyValues of the latest map (grid_map.cpp:439-457) */
    std::vector<std::uint16_t> CopyLatestMapValues() const
    {
        std::vector<std::uint16_t> values(static_cast<std::size_t>(this->mShape.rows) * this->mShape.cols);
        CSM_ASSERT_OK(this->mCtx, csm_download_level(this->mCtx, this->mLatestMap.mId, 0, values.data()));
        return values;
    }

    /* A new, empty local map on the device: GridMap(resolution, patchSize, 1.0, 1.0)
     * as UpdatePoseGraph creates it (grid_map_builder.cpp:251) */
    void CreateLocalMap(std::uint64_t localMapId)
    {
        const csm_map_shape shape = this->FreshShape();
        const std::vector<std::uint16_t> empty(static_cast<std::size_t>(shape.rows) * shape.cols, 0);
        CSM_ASSERT_OK(this->mCtx, csm_upload_grid(this->mCtx, localMapId, empty.data(), shape.rows, shape.cols));
        this->mLocalShapes[localMapId] = shape;
    }

    /* the grid half of GridMapBuilder::UpdateGridMap (grid_map_builder.cpp:389-494):
     * the latest scan node into the local map that is being built */
    void UpdateGridMap(std::uint64_t localMapId, const RobotPose2D<double>& globalMapPose,
                       const ScanNodeView& latestScanNode)
    {
        auto it = this->mLocalShapes.find(localMapId);
        CSM_ASSERT_THAT(it != this->mLocalShapes.end(), "local map %llu exists",
                        static_cast<unsigned long long>(localMapId));
        const csm_scan_node flat = detail::ToScanNode(latestScanNode);
        const double pose[3] = { globalMapPose.mX, globalMapPose.mY, globalMapPose.mTheta };
        CSM_ASSERT_OK(this->mCtx, csm_update_map_with_scan(this->mCtx, localMapId, &it->second, pose, &flat,
                                                           &this->mParams, &this->mInfo));
    }

    /* What GridMapBuilder::AfterLoopClosure announces ("Re-create the local grid maps and latest map
     * after the loop closure", grid_map_builder.cpp:134) and leaves undone: the listed local maps are
     * rebuilt from their scan nodes (whose poses the optimization has moved) in one call
     * (csm_construct_maps_from_scans), each in the frame it had. nodeSpans[i] = the scan nodes of local
     * map localMapIds[i] in id order; a local map that does not exist yet is created first. LocalMap(id)
     * returns the new geometry afterwards. Any job's failure is an assertion, as in the single build. */
    void ConstructLocalMaps(const std::vector<std::uint64_t>& localMapIds,
                            const std::vector<RobotPose2D<double>>& globalMapPoses,
                            const std::vector<std::pair<const ScanNodeView*, std::size_t>>& nodeSpans)
    {
        CSM_ASSERT_THAT(!localMapIds.empty() && globalMapPoses.size() == localMapIds.size() &&
                            nodeSpans.size() == localMapIds.size(),
                        "one pose and one node span per local map");
        std::vector<std::vector<csm_scan_node>> flat(localMapIds.size());
        std::vector<csm_map_build_job> jobs(localMapIds.size());
        for (std::size_t m = 0; m < localMapIds.size(); ++m) {
            if (this->mLocalShapes.find(localMapIds[m]) == this->mLocalShapes.end())
                this->CreateLocalMap(localMapIds[m]);
            flat[m] = detail::ToScanNodes(nodeSpans[m].first, nodeSpans[m].second);
            csm_map_build_job& job = jobs[m];
            job = csm_map_build_job {};
            job.map_id = localMapIds[m];
            job.shape = this->mLocalShapes.at(localMapIds[m]);
            job.global_map_pose[0] = globalMapPoses[m].mX;
            job.global_map_pose[1] = globalMapPoses[m].mY;
            job.global_map_pose[2] = globalMapPoses[m].mTheta;
            job.nodes = flat[m].data();
            job.n_nodes = static_cast<std::int32_t>(flat[m].size());
        }
        CSM_ASSERT_OK(this->mCtx, csm_construct_maps_from_scans(this->mCtx, jobs.data(),
                                                                static_cast<std::int32_t>(jobs.size()),
                                                                &this->mParams, nullptr, &this->mBatchInfo));
        for (const csm_map_build_job& job : jobs)
            this->mLocalShapes[job.map_id] = job.shape;
    }
    const csm_map_batch_info& LastBatchInfo() const { return this->mBatchInfo; }

    /* GridMapBuilder::ConstructGlobalMap (grid_map_builder.cpp:162-184): one map of all scan nodes of
     * the pose graph (in id order), on the device under globalMapId (csm_construct_global_map: cast in
     * parts, long hit lists sorted). The map pose is the first node's global pose (:171-172); the map
     * is fresh, as GridMap{res, patchSize, 1.0, 1.0} at :175. globalMapPose and shape are set;
     * LocalMap(globalMapId) and CopyLocalMapValues(globalMapId) read the result. */
    void ConstructGlobalMap(std::uint64_t globalMapId, const ScanNodeView* nodes, std::size_t numOfNodes,
                            RobotPose2D<double>& globalMapPose, csm_map_shape& shape)
    {
        CSM_ASSERT_THAT(nodes != nullptr && numOfNodes != 0, "!scanNodes.empty()");
        const std::vector<csm_scan_node> flat = detail::ToScanNodes(nodes, numOfNodes);
        globalMapPose = nodes[0].mGlobalPose;
        const double pose[3] = { globalMapPose.mX, globalMapPose.mY, globalMapPose.mTheta };
        shape = this->FreshShape();
        CSM_ASSERT_OK(this->mCtx, csm_construct_global_map(
                                      this->mCtx, globalMapId, &shape, pose, flat.data(),
                                      static_cast<std::int32_t>(numOfNodes), &this->mParams, &this->mGlobalParams,
                                      &this->mInfo, &this->mGlobalInfo));
        this->mLocalShapes[globalMapId] = shape;
    }
    /* scratch limit and rank settings of ConstructGlobalMap (zeros: the library's defaults) */
    void SetGlobalMapParams(const csm_global_map_params& params) { this->mGlobalParams = params; }
    const csm_global_map_info& LastGlobalMapInfo() const { return this->mGlobalInfo; }

    /* geometry + id of a local map (cells on the device), e.g. for a LoopDetectionQuery */
    GridMapView LocalMap(std::uint64_t localMapId) const
    {
        return detail::ToView(this->mLocalShapes.at(localMapId), localMapId);
    }

    std::vector<std::uint16_t> CopyLocalMapValues(std::uint64_t localMapId) const
    {
        const csm_map_shape& shape = this->mLocalShapes.at(localMapId);
        std::vector<std::uint16_t> values(static_cast<std::size_t>(shape.rows) * shape.cols);
        CSM_ASSERT_OK(this->mCtx, csm_download_level(this->mCtx, localMapId, 0, values.data()));
        return values;
    }

private:
    void SyncView() { this->mLatestMap = detail::ToView(this->mShape, this->mLatestMap.mId); }

    /* the shape of a new map: GridMap(resolution, patchSize, 1.0, 1.0), as the constructor computed it */
    csm_map_shape FreshShape() const
    {
        csm_map_shape shape = this->mShape;
        shape.offset_x = shape.offset_y = 0.0;
        shape.rows = shape.cols = this->mInitialCells;
        return shape;
    }

    csm_ctx* mCtx;
    int mNumOfScansForLatestMap;
    RobotPose2D<double> mLatestMapPose;
    csm_map_builder_params mParams {};
    csm_map_shape mShape {};
    csm_map_build_info mInfo {};
    csm_map_batch_info mBatchInfo {};
    csm_global_map_params mGlobalParams {};
    csm_global_map_info mGlobalInfo {};
    GridMapView mLatestMap;
    int mInitialCells = 0;
    std::map<std::uint64_t, csm_map_shape> mLocalShapes;
};

/* EdgePose (inc/mapping/pose_graph_edge.hpp:131-157) with the Eigen members restated as arrays:
 * mRelativePose = { x, y, theta }, mInformationMat row-major */
struct EdgePose {
    bool mIsLoopConstraint;
    int mLocalMapNodeIdx;
    int mScanNodeIdx;
    std::array<double, 3> mRelativePose;
    std::array<double, 9> mInformationMat;
};

/* A (local map node, scan node) pair whose marginal covariance is asked for; mScanNodeIdx = -1: the
 * local map node alone */
struct NodePair {
    int mLocalMapNodeIdx;
    int mScanNodeIdx;
};

/* csm_pose_graph_marginal with the blocks as row-major arrays */
struct PairMarginal {
    std::array<double, 9> localCov;
    std::array<double, 9> scanCov;
    std::array<double, 9> crossCov;
    std::array<double, 9> relativeCov;
    bool finite;
};

/* The loop search window (range x, y, theta: full widths in the local map's frame) from a pair's
 * relativeCov: 2 nSigma standard deviations, clamped (csm_host_loop_search_ranges). Returns false for
 * what that function refuses. */
inline bool LoopSearchRanges(const std::array<double, 9>& relativeCov, double nSigma,
                             const std::array<double, 3>& minRange, const std::array<double, 3>& maxRange,
                             std::array<double, 3>& ranges)
{
    return csm_host_loop_search_ranges(relativeCov.data(), nSigma, minRange.data(), maxRange.data(),
                                       ranges.data()) == CSM_OK;
}

/* The gate of a found loop against the graph's prediction: chi2 = d^T (relativeCov + matchCov)^-1 d with
 * d = measured - predicted (csm_host_loop_gate). Returns false when the sum is not positive definite. */
inline bool LoopGate(const std::array<double, 9>& relativeCov, const std::array<double, 9>& matchCov,
                     const std::array<double, 3>& predicted, const std::array<double, 3>& measured, double& chi2)
{
    return csm_host_loop_gate(relativeCov.data(), matchCov.data(), predicted.data(), measured.data(), &chi2) ==
           CSM_OK;
}

/* PoseGraphOptimizerLM (inc/mapping/pose_graph_optimizer_lm.hpp:84-160) on the device. Create()
 * takes the constructor's arguments with the loss function as (CSM_PG_LOSS_*, scale); it returns null
 * for SolverType SparseCholesky (SimplicialLDLT: not provided; SchurCholesky is the direct solver that
 * is), NumOfIterationsMax < 1 or no device. mLambda is kept
 * between Optimize calls, as the reference's member is. Node poses are { x, y, theta } in place of
 * Eigen::Vector3d. */
class PoseGraphOptimizerLMHIP final {
public:
    enum class SolverType { SparseCholesky, ConjugateGradient, SchurCholesky };

    static std::unique_ptr<PoseGraphOptimizerLMHIP> Create(SolverType solverType, int numOfIterationsMax,
                                                           double errorTolerance, double initialLambda,
                                                           int lossType, double lossScale, int deviceId = 0)
    {
        if ((solverType != SolverType::ConjugateGradient && solverType != SolverType::SchurCholesky) ||
            numOfIterationsMax < 1)
            return nullptr;
        detail::CtxPtr ctx = detail::MakeContext(deviceId);
        if (!ctx)
            return nullptr;
        csm_pose_graph_lm_params prm {};
        prm.iterations_max = numOfIterationsMax;
        prm.solver_type = solverType == SolverType::SchurCholesky ? CSM_PG_SOLVER_SCHUR_CHOLESKY
                                                                  : CSM_PG_SOLVER_CONJUGATE_GRADIENT;
        prm.loss_type = lossType;
        prm.error_tolerance = errorTolerance;
        prm.loss_scale = lossScale;
        return std::unique_ptr<PoseGraphOptimizerLMHIP>(
            new PoseGraphOptimizerLMHIP(prm, initialLambda, std::move(ctx)));
    }

    PoseGraphOptimizerLMHIP(const PoseGraphOptimizerLMHIP&) = delete;
    PoseGraphOptimizerLMHIP& operator=(const PoseGraphOptimizerLMHIP&) = delete;

    csm_ctx* Context() const { return this->mCtx.get(); }
    double Lambda() const { return this->mLambda; }
    /* the metrics of the last call (PoseGraphOptimizerLMMetrics: NumOfIterations, InitialError, FinalError) */
    const csm_pose_graph_lm_info& LastInfo() const { return this->mLast; }

    void Optimize(std::vector<std::array<double, 3>>& localMapNodes, std::vector<std::array<double, 3>>& scanNodes,
                  const std::vector<EdgePose>& poseGraphEdges)
    {
        this->FillEdges(poseGraphEdges);
        /* std::array<double, 3> is three contiguous doubles: the vectors are the flat pose arrays */
        static_assert(sizeof(std::array<double, 3>) == 3 * sizeof(double), "pose layout");
        CSM_ASSERT_OK(this->mCtx.get(),
                      csm_pose_graph_lm(this->mCtx.get(), localMapNodes.empty() ? nullptr : localMapNodes.front().data(),
                                        static_cast<std::int32_t>(localMapNodes.size()),
                                        scanNodes.empty() ? nullptr : scanNodes.front().data(),
                                        static_cast<std::int32_t>(scanNodes.size()), this->mEdges.data(),
                                        static_cast<std::int32_t>(this->mEdges.size()), &this->mParams,
                                        &this->mLambda, &this->mLast, nullptr));
    }

    /* The marginal covariances of the pairs at the given poses, under the optimizer's loss function
     * (csm_pose_graph_marginals): how uncertain the graph is about each pair. */
    std::vector<PairMarginal> ComputeMarginals(const std::vector<std::array<double, 3>>& localMapNodes,
                                               const std::vector<std::array<double, 3>>& scanNodes,
                                               const std::vector<EdgePose>& poseGraphEdges,
                                               const std::vector<NodePair>& pairs)
    {
        this->FillEdges(poseGraphEdges);
        std::vector<csm_pose_graph_pair> cp(pairs.size());
        for (std::size_t i = 0; i < pairs.size(); ++i)
            cp[i] = csm_pose_graph_pair { pairs[i].mLocalMapNodeIdx, pairs[i].mScanNodeIdx };
        std::vector<csm_pose_graph_marginal> rec(pairs.size());
        CSM_ASSERT_OK(this->mCtx.get(),
                      csm_pose_graph_marginals(this->mCtx.get(),
                                               localMapNodes.empty() ? nullptr : localMapNodes.front().data(),
                                               static_cast<std::int32_t>(localMapNodes.size()),
                                               scanNodes.empty() ? nullptr : scanNodes.front().data(),
                                               static_cast<std::int32_t>(scanNodes.size()), this->mEdges.data(),
                                               static_cast<std::int32_t>(this->mEdges.size()), this->mParams.loss_type,
                                               this->mParams.loss_scale, cp.data(),
                                               static_cast<std::int32_t>(cp.size()), rec.data(), nullptr));
        std::vector<PairMarginal> out(rec.size());
        for (std::size_t i = 0; i < rec.size(); ++i) {
            std::copy(rec[i].local_cov, rec[i].local_cov + 9, out[i].localCov.begin());
            std::copy(rec[i].scan_cov, rec[i].scan_cov + 9, out[i].scanCov.begin());
            std::copy(rec[i].cross_cov, rec[i].cross_cov + 9, out[i].crossCov.begin());
            std::copy(rec[i].relative_cov, rec[i].relative_cov + 9, out[i].relativeCov.begin());
            out[i].finite = rec[i].finite != 0;
        }
        return out;
    }

private:
    PoseGraphOptimizerLMHIP(const csm_pose_graph_lm_params& prm, double lambda, detail::CtxPtr ctx) :
        mParams(prm), mLambda(lambda), mCtx(std::move(ctx)) { }

    void FillEdges(const std::vector<EdgePose>& poseGraphEdges)
    {
        this->mEdges.resize(poseGraphEdges.size());
        for (std::size_t i = 0; i < poseGraphEdges.size(); ++i) {
            const EdgePose& e = poseGraphEdges[i];
            csm_pose_graph_edge& d = this->mEdges[i];
            d = csm_pose_graph_edge {};
            d.local_map_index = e.mLocalMapNodeIdx;
            d.scan_index = e.mScanNodeIdx;
            d.is_loop = e.mIsLoopConstraint ? 1 : 0;
            for (int j = 0; j < 3; ++j)
                d.relative_pose[j] = e.mRelativePose[j];
            for (int j = 0; j < 9; ++j)
                d.information[j] = e.mInformationMat[j];
        }
    }

    const csm_pose_graph_lm_params mParams;
    double mLambda;
    detail::CtxPtr mCtx;
    std::vector<csm_pose_graph_edge> mEdges;
    csm_pose_graph_lm_info mLast {};
};

/* The drift model of LoopConsistencyHIP: variances per metre travelled and the accumulated travel distance at
 * every node (a local map takes the value of its first scan node). */
struct LoopDriftModel {
    std::array<double, 3> mVariancePerMetre;
    std::vector<double> mLocalMapTravel;
    std::vector<double> mScanTravel;
};

/* Do the loop edges agree with each other (csm_loop_consistency)? Sits in RunStep between Detect and
 * AppendLoopClosingEdges: Check() tests every pair of candidate edges at the graph's current poses and finds the
 * largest set that is pairwise consistent; SelectConsistent() keeps that subset of the detector's results. Nodes
 * and edges are taken as PoseGraphOptimizerLMHIP takes them. The library has no such class in the reference. */
class LoopConsistencyHIP final {
public:
    /* gate: the chi-square bound of a pair's cycle (11.34 = 99 % of three degrees of freedom); numOfSeeds: greedy
     * searches from the vertices of highest degree, 0 = from every vertex */
    static std::unique_ptr<LoopConsistencyHIP> Create(double gate, int numOfSeeds = 0, int deviceId = 0)
    {
        if (!(gate >= 0.0) || numOfSeeds < 0)
            return nullptr;
        detail::CtxPtr ctx = detail::MakeContext(deviceId);
        if (!ctx)
            return nullptr;
        return std::unique_ptr<LoopConsistencyHIP>(
            new LoopConsistencyHIP(gate, numOfSeeds, detail::ContextRef(std::move(ctx))));
    }
    /* on a context another adapter owns and keeps alive */
    LoopConsistencyHIP(csm_ctx* shared, double gate, int numOfSeeds = 0) :
        LoopConsistencyHIP(gate, numOfSeeds, detail::ContextRef(shared)) { }

    LoopConsistencyHIP(const LoopConsistencyHIP&) = delete;
    LoopConsistencyHIP& operator=(const LoopConsistencyHIP&) = delete;

    csm_ctx* Context() const { return this->mCtx.Get(); }
    /* the records of the last Check: one flag and one degree per edge, and the totals */
    const std::vector<std::int32_t>& Selected() const { return this->mSelected; }
    const std::vector<std::int32_t>& Degree() const { return this->mDegree; }
    const csm_loop_consistency_info& LastInfo() const { return this->mLastInfo; }

    void Check(const std::vector<std::array<double, 3>>& localMapNodes,
               const std::vector<std::array<double, 3>>& scanNodes, const std::vector<EdgePose>& loopEdges,
               const LoopDriftModel* drift = nullptr)
    {
        std::vector<csm_pose_graph_edge> edges(loopEdges.size());
        for (std::size_t i = 0; i < loopEdges.size(); ++i) {
            const EdgePose& e = loopEdges[i];
            csm_pose_graph_edge& d = edges[i];
            d = csm_pose_graph_edge {};
            d.local_map_index = e.mLocalMapNodeIdx;
            d.scan_index = e.mScanNodeIdx;
            d.is_loop = e.mIsLoopConstraint ? 1 : 0;
            std::copy(e.mRelativePose.begin(), e.mRelativePose.end(), d.relative_pose);
            std::copy(e.mInformationMat.begin(), e.mInformationMat.end(), d.information);
        }
        this->Run(localMapNodes, scanNodes, edges, drift);
    }

    /* the same on a detector's results: z = the estimated map-local pose, Lambda = the inverse of the estimated
     * covariance (csm_host_information_from_covariance), the local map node and scan node by their ids */
    void Check(const std::vector<std::array<double, 3>>& localMapNodes,
               const std::vector<std::array<double, 3>>& scanNodes, const LoopDetectionResultVector& results,
               const LoopDriftModel* drift = nullptr)
    {
        std::vector<csm_pose_graph_edge> edges(results.size());
        for (std::size_t i = 0; i < results.size(); ++i) {
            const LoopDetectionResult& r = results[i];
            csm_pose_graph_edge& d = edges[i];
            d = csm_pose_graph_edge {};
            d.local_map_index = static_cast<std::int32_t>(r.mLocalMapNodeId);
            d.scan_index = r.mScanNodeId;
            d.is_loop = 1;
            d.relative_pose[0] = r.mRelativePose.mX;
            d.relative_pose[1] = r.mRelativePose.mY;
            d.relative_pose[2] = r.mRelativePose.mTheta;
            CSM_ASSERT_OK(this->Context(), csm_host_information_from_covariance(r.mEstimatedCovariance, d.information));
        }
        this->Run(localMapNodes, scanNodes, edges, drift);
    }

    /* the results the last Check selected, in their original order; `results` is what that Check was given */
    LoopDetectionResultVector SelectConsistent(const LoopDetectionResultVector& results) const
    {
        CSM_ASSERT_THAT(results.size() == this->mSelected.size(), "%zu results, but the last Check saw %zu edges",
                        results.size(), this->mSelected.size());
        LoopDetectionResultVector kept;
        for (std::size_t i = 0; i < results.size(); ++i)
            if (this->mSelected[i])
                kept.push_back(results[i]);
        return kept;
    }

private:
    LoopConsistencyHIP(double gate, int numOfSeeds, detail::ContextRef ctx) :
        mGate(gate), mNumOfSeeds(numOfSeeds), mCtx(std::move(ctx)) { }

    void Run(const std::vector<std::array<double, 3>>& localMapNodes,
             const std::vector<std::array<double, 3>>& scanNodes, const std::vector<csm_pose_graph_edge>& edges,
             const LoopDriftModel* drift)
    {
        static_assert(sizeof(std::array<double, 3>) == 3 * sizeof(double), "pose layout");
        if (drift)
            CSM_ASSERT_THAT(drift->mLocalMapTravel.size() == localMapNodes.size() &&
                            drift->mScanTravel.size() == scanNodes.size(), "%s", "one travel distance per node");
        this->mSelected.assign(edges.size(), 0);
        this->mDegree.assign(edges.size(), 0);
        CSM_ASSERT_OK(this->Context(),
                      csm_loop_consistency(this->Context(), localMapNodes.empty() ? nullptr : localMapNodes.front().data(),
                                           static_cast<std::int32_t>(localMapNodes.size()),
                                           scanNodes.empty() ? nullptr : scanNodes.front().data(),
                                           static_cast<std::int32_t>(scanNodes.size()), edges.data(),
                                           static_cast<std::int32_t>(edges.size()), this->mGate,
                                           drift ? drift->mVariancePerMetre.data() : nullptr,
                                           drift ? drift->mLocalMapTravel.data() : nullptr,
                                           drift ? drift->mScanTravel.data() : nullptr, this->mNumOfSeeds,
                                           this->mSelected.data(), this->mDegree.data(), &this->mLastInfo, nullptr,
                                           nullptr));
    }

    const double mGate;
    const int mNumOfSeeds;
    detail::ContextRef mCtx;
    std::vector<std::int32_t> mSelected, mDegree;
    csm_loop_consistency_info mLastInfo {};
};

/* ScoreFunction::Summary (inc/mapping/score_function.hpp:29-45) plus the integers it came from */
struct ScoreSummary {
    double mNormalizedScore = 0.0;
    double mScore = 0.0;
    double mKnownRate = 0.0;
    std::uint32_t mSumValues = 0, mKnown = 0, mFlags = 0;
};

/* ScorePixelAccurate (inc/mapping/score_function_pixel_accurate.hpp, src/mapping/
 * score_function_pixel_accurate.cpp:16-58) on the device: Score(gridMap, scan, mapLocalSensorPose) for a
 * resident map, at one pose or at many in one launch chain (csm_score_pose_sets). The doubles come from
 * the integer sums through csm_host_score_from_sums: within 1e-12 of the reference's beam-order sum. A map is
 * made resident with Upload() or by any other adapter that shares the context. */
class ScorePixelAccurateHIP final {
public:
    static std::unique_ptr<ScorePixelAccurateHIP> Create(int deviceId = 0)
    {
        detail::CtxPtr ctx = detail::MakeContext(deviceId);
        if (!ctx)
            return nullptr;
        return std::unique_ptr<ScorePixelAccurateHIP>(new ScorePixelAccurateHIP(detail::ContextRef(std::move(ctx))));
    }
    /* on a context another adapter owns (and keeps alive) */
    explicit ScorePixelAccurateHIP(csm_ctx* shared) : mCtx(shared) { }

    ScorePixelAccurateHIP(const ScorePixelAccurateHIP&) = delete;
    ScorePixelAccurateHIP& operator=(const ScorePixelAccurateHIP&) = delete;

    csm_ctx* Context() const { return this->mCtx.Get(); }
    const csm_pose_sets_info& LastInfo() const { return this->mLast; }

    void Upload(const GridMapView& g)
    {
        CSM_ASSERT_OK(this->Context(), csm_upload_grid(this->Context(), g.mId, g.mValues, g.mRows, g.mCols));
    }

    ScoreSummary Score(std::uint64_t mapId, const csm_geometry& geometry, const ScanDataView& scan,
                       const RobotPose2D<double>& mapLocalSensorPose)
    {
        return this->ScoreMany(mapId, geometry, scan, { mapLocalSensorPose }).front();
    }

    std::vector<ScoreSummary> ScoreMany(std::uint64_t mapId, const csm_geometry& geometry, const ScanDataView& scan,
                                        const std::vector<RobotPose2D<double>>& mapLocalSensorPoses)
    {
        const csm_pose_set set = detail::ToPoseSet(mapId, geometry, scan, mapLocalSensorPoses);
        std::vector<csm_pose_record> rec(mapLocalSensorPoses.size());
        CSM_ASSERT_OK(this->Context(), csm_score_pose_sets(this->Context(), &set, 1, rec.data(), &this->mLast));
        std::vector<ScoreSummary> out(rec.size());
        for (std::size_t i = 0; i < rec.size(); ++i) {
            ScoreSummary& o = out[i];
            CSM_ASSERT_OK(this->Context(), csm_host_score_from_sums(rec[i].sum_values, rec[i].known, set.scan.n_points,
                                                                    &o.mNormalizedScore, &o.mKnownRate));
            o.mScore = o.mNormalizedScore * static_cast<double>(set.scan.n_points);
            o.mSumValues = rec[i].sum_values;
            o.mKnown = rec[i].known;
            o.mFlags = rec[i].flags;
        }
        return out;
    }

    /* The same for map-local ROBOT poses: the scan's relative sensor pose is applied on the host
     * (Compound, inc/pose.hpp:154-166), as the matchers do before they score. */
    std::vector<ScoreSummary> ScoreManyRobotPoses(std::uint64_t mapId, const csm_geometry& geometry,
                                                  const ScanDataView& scan,
                                                  const std::vector<RobotPose2D<double>>& mapLocalRobotPoses)
    {
        return this->ScoreMany(mapId, geometry, scan, SensorPoses(scan, mapLocalRobotPoses));
    }

    static std::vector<RobotPose2D<double>> SensorPoses(const ScanDataView& scan,
                                                        const std::vector<RobotPose2D<double>>& robotPoses)
    {
        const double rel[3] = { scan.mRelativeSensorPose.mX, scan.mRelativeSensorPose.mY,
                                scan.mRelativeSensorPose.mTheta };
        std::vector<RobotPose2D<double>> out(robotPoses.size());
        for (std::size_t i = 0; i < robotPoses.size(); ++i) {
            const double p[3] = { robotPoses[i].mX, robotPoses[i].mY, robotPoses[i].mTheta };
            double s[3];
            csm_host_compound(p, rel, s);
            out[i] = { s[0], s[1], s[2] };
        }
        return out;
    }

private:
    explicit ScorePixelAccurateHIP(detail::ContextRef ctx) : mCtx(std::move(ctx)) { }

    detail::ContextRef mCtx;
    csm_pose_sets_info mLast {};
};

/* The measurement update of a particle filter that localises in a finished map (beyond the reference, which
 * has no such filter): every particle's sensor pose scored against the map or its likelihood field, integer
 * weights exp(-(score_max - score) / temperature) in 2^-24 units and a systematically resampled set, all in
 * one launch chain (csm_pose_set_update). */
class ParticleSetHIP final {
public:
    struct Update {
        std::vector<csm_pose_record> mRecords;
        std::vector<std::uint32_t> mWeights;
        std::vector<std::int32_t> mAncestors;      /* index of the particle each output copies, -1: none */
        double mEffectiveSampleSize = 0.0;         /* (sum w)^2 / sum w^2 in double, on the host */
        csm_pose_update_info mUpdate {};
        csm_pose_sets_info mInfo {};
    };

    static std::unique_ptr<ParticleSetHIP> Create(double temperature, double knownRateThreshold, int deviceId = 0)
    {
        detail::CtxPtr ctx = detail::MakeContext(deviceId);
        if (!ctx)
            return nullptr;
        return std::unique_ptr<ParticleSetHIP>(
            new ParticleSetHIP(temperature, knownRateThreshold, detail::ContextRef(std::move(ctx))));
    }
    ParticleSetHIP(csm_ctx* shared, double temperature, double knownRateThreshold) :
        ParticleSetHIP(temperature, knownRateThreshold, detail::ContextRef(shared)) { }

    ParticleSetHIP(const ParticleSetHIP&) = delete;
    ParticleSetHIP& operator=(const ParticleSetHIP&) = delete;

    csm_ctx* Context() const { return this->mCtx.Get(); }

    /* `offset` places the comb of the systematic resampling: any 64-bit draw of the caller's generator */
    Update MeasurementUpdate(std::uint64_t mapId, const csm_geometry& geometry, const ScanDataView& scan,
                             const std::vector<RobotPose2D<double>>& mapLocalSensorPoses, std::size_t numOfOutputs,
                             std::uint64_t offset)
    {
        const csm_pose_set set = detail::ToPoseSet(mapId, geometry, scan, mapLocalSensorPoses);
        csm_pose_update_params prm {};
        prm.temperature = this->mTemperature;
        prm.known_rate_threshold = this->mKnownRateThreshold;
        prm.n_out = static_cast<std::int32_t>(numOfOutputs);
        prm.offset = offset;
        Update out;
        out.mRecords.resize(mapLocalSensorPoses.size());
        out.mWeights.resize(mapLocalSensorPoses.size());
        out.mAncestors.resize(numOfOutputs);
        CSM_ASSERT_OK(this->Context(), csm_pose_set_update(this->Context(), &set, &prm, out.mRecords.data(),
                                                           out.mWeights.data(), out.mAncestors.data(), &out.mUpdate,
                                                           &out.mInfo));
        double sum = 0.0, sumSq = 0.0;
        for (std::uint32_t w : out.mWeights) {
            sum += static_cast<double>(w);
            sumSq += static_cast<double>(w) * static_cast<double>(w);
        }
        out.mEffectiveSampleSize = sumSq > 0.0 ? sum * sum / sumSq : 0.0;
        return out;
    }

private:
    ParticleSetHIP(double temperature, double knownRateThreshold, detail::ContextRef ctx) :
        mTemperature(temperature), mKnownRateThreshold(knownRateThreshold), mCtx(std::move(ctx)) { }

    const double mTemperature, mKnownRateThreshold;
    detail::ContextRef mCtx;
};

/* The settings of a cast (csm_ray_cast_params). Create: occupied at P >= probOccupied (above 0.5), the raw
 * value the ray check would use (csm_host_ray_check_values). */
struct RayCastSettings {
    double mRangeMax = 20.0, mRangeMin = 0.0;
    int mSubpixelScale = 100;
    std::uint32_t mOccupiedMin = 0;
    bool mUnknownStops = false;
    double mNoneValue = 0.0;             /* the range reported for a beam that did not stop */

    static RayCastSettings Create(double rangeMax = 20.0, double rangeMin = 0.0, double probOccupied = 0.65,
                                  bool unknownStops = false, int subpixelScale = 100)
    {
        RayCastSettings s;
        s.mRangeMax = rangeMax;
        s.mRangeMin = rangeMin;
        s.mSubpixelScale = subpixelScale;
        s.mUnknownStops = unknownStops;
        std::uint32_t freeMax = 0;
        CSM_ASSERT_OK(nullptr, csm_host_ray_check_values(probOccupied, 1.0 - probOccupied, &s.mOccupiedMin, &freeMax));
        return s;
    }
    csm_ray_cast_params Params() const
    {
        csm_ray_cast_params p {};
        p.range_max = this->mRangeMax;
        p.range_min = this->mRangeMin;
        p.subpixel_scale = this->mSubpixelScale;
        p.occupied_min = this->mOccupiedMin;
        p.unknown_stops = this->mUnknownStops ? 1 : 0;
        return p;
    }
};

/* A scan that owns its beams (ScanDataView points into it). */
struct VirtualScan {
    std::vector<double> mAngles, mRanges;
    ScanDataView View() const
    {
        ScanDataView v;
        v.mAngles = this->mAngles.data();
        v.mRanges = this->mRanges.data();
        v.mNumOfScans = this->mAngles.size();
        return v;
    }
};

/* Virtual scans (beyond the reference, which only ever walks a measured beam): from map-local sensor poses,
 * in the directions of `angles`, the first cell of a resident map that stops each beam and its distance
 * (csm_ray_cast; the ranges from csm_host_ray_cast_ranges). ScanFromMap gives the stopped beams of one pose as
 * a scan with a zero relative sensor pose: a finished local map seen from its centre can then go through the
 * descriptors, the matchers and the ray check like any scan node. A map is made resident with Upload() or by
 * any other adapter that shares the context. */
class VirtualScanHIP final {
public:
    struct Casts {
        std::vector<csm_ray_cast_record> mRecords;     /* [poses][angles] */
        std::vector<double> mRanges;                   /* likewise; mNoneValue where a beam did not stop */
        csm_ray_cast_info mInfo {};
    };

    static std::unique_ptr<VirtualScanHIP> Create(int deviceId = 0)
    {
        detail::CtxPtr ctx = detail::MakeContext(deviceId);
        if (!ctx)
            return nullptr;
        return std::unique_ptr<VirtualScanHIP>(new VirtualScanHIP(detail::ContextRef(std::move(ctx))));
    }
    /* on a context another adapter owns (and keeps alive) */
    explicit VirtualScanHIP(csm_ctx* shared) : mCtx(shared) { }

    VirtualScanHIP(const VirtualScanHIP&) = delete;
    VirtualScanHIP& operator=(const VirtualScanHIP&) = delete;

    csm_ctx* Context() const { return this->mCtx.Get(); }

    void Upload(const GridMapView& g)
    {
        CSM_ASSERT_OK(this->Context(), csm_upload_grid(this->Context(), g.mId, g.mValues, g.mRows, g.mCols));
    }

    Casts Cast(std::uint64_t mapId, const csm_geometry& geometry,
               const std::vector<RobotPose2D<double>>& mapLocalSensorPoses, const std::vector<double>& angles,
               const RayCastSettings& settings)
    {
        ScanDataView beams;
        beams.mAngles = angles.data();
        beams.mNumOfScans = angles.size();
        const csm_pose_set set = detail::ToPoseSet(mapId, geometry, beams, mapLocalSensorPoses);
        const csm_ray_cast_params prm = settings.Params();
        Casts out;
        out.mRecords.resize(mapLocalSensorPoses.size() * angles.size());
        out.mRanges.resize(out.mRecords.size());
        CSM_ASSERT_OK(this->Context(), csm_ray_cast(this->Context(), &set, 1, &prm, out.mRecords.data(), &out.mInfo));
        CSM_ASSERT_OK(this->Context(), csm_host_ray_cast_ranges(out.mRecords.data(),
                                                                static_cast<std::int64_t>(out.mRecords.size()),
                                                                geometry.resolution, prm.subpixel_scale,
                                                                settings.mNoneValue, out.mRanges.data()));
        return out;
    }

    /* the beams of one pose that stopped, in beam order */
    VirtualScan ScanFromMap(std::uint64_t mapId, const csm_geometry& geometry,
                            const RobotPose2D<double>& mapLocalSensorPose, const std::vector<double>& angles,
                            const RayCastSettings& settings)
    {
        const Casts casts = this->Cast(mapId, geometry, { mapLocalSensorPose }, angles, settings);
        VirtualScan scan;
        for (std::size_t i = 0; i < angles.size(); ++i)
            if (casts.mRecords[i].kind != CSM_CAST_NONE) {
                scan.mAngles.push_back(angles[i]);
                scan.mRanges.push_back(casts.mRanges[i]);
            }
        return scan;
    }

private:
    explicit VirtualScanHIP(detail::ContextRef ctx) : mCtx(std::move(ctx)) { }

    detail::ContextRef mCtx;
};

/* What LoopSearcherNearest::Search reads of LoopSearchHint (inc/mapping/loop_searcher.hpp:25-53): the global
 * poses of the finished scan nodes ({ x, y, theta }, node i = NodeId i), every local map's
 * (mScanNodeIdMin, mScanNodeIdMax) -- contiguous runs from node 0 -- the accumulated travel distance and the
 * id of the last finished local map. */
struct LoopSearchHintView {
    const std::array<double, 3>* mScanNodePoses = nullptr;
    std::size_t mNumOfScanNodes = 0;
    const std::pair<int, int>* mLocalMapNodeRanges = nullptr;
    std::size_t mNumOfLocalMaps = 0;
    double mAccumTravelDist = 0.0;
    int mLastFinishedMapId = -1;
};

namespace detail {

/* a hint as the arrays a loop search takes: the nodes up to the last finished map's last, the map of each,
 * their travel distances; mNumOfRefs = the first node of the last finished map */
struct LoopGraph {
    std::int32_t mNumOfNodes = 0, mNumOfMaps = 0, mNumOfRefs = 0;
    std::vector<std::int32_t> mMapIndex;
    std::vector<double> mTravel;
};

inline LoopGraph ToLoopGraph(const LoopSearchHintView& h, csm_ctx* ctx)
{
    CSM_ASSERT_THAT(h.mLastFinishedMapId >= 0 && static_cast<std::size_t>(h.mLastFinishedMapId) < h.mNumOfLocalMaps,
                    "mLastFinishedMapId names no local map");
    LoopGraph g;
    g.mNumOfMaps = h.mLastFinishedMapId + 1;
    for (std::int32_t m = 0; m < g.mNumOfMaps; ++m) {
        const std::pair<int, int>& run = h.mLocalMapNodeRanges[m];
        CSM_ASSERT_THAT(run.first == g.mNumOfNodes && run.second >= run.first,
                        "local maps must be contiguous runs of scan nodes from node 0");
        if (m == h.mLastFinishedMapId)
            g.mNumOfRefs = g.mNumOfNodes;
        g.mMapIndex.insert(g.mMapIndex.end(), static_cast<std::size_t>(run.second - run.first + 1), m);
        g.mNumOfNodes = run.second + 1;
    }
    CSM_ASSERT_THAT(static_cast<std::size_t>(g.mNumOfNodes) <= h.mNumOfScanNodes,
                    "a local map names a scan node that is not given");
    g.mTravel.resize(static_cast<std::size_t>(g.mNumOfNodes));
    static_assert(sizeof(std::array<double, 3>) == 3 * sizeof(double), "pose layout");
    CSM_ASSERT_OK(ctx, csm_host_travel_distances(h.mScanNodePoses->data(), g.mNumOfNodes, g.mTravel.data()));
    return g;
}

} /* namespace detail */

/* inc/mapping/loop_searcher.hpp:63-85, plus the squared node distance the searcher observes as a metric */
struct LoopCandidate {
    int mQueryScanNodeId;
    int mReferenceScanNodeId;
    int mReferenceLocalMapId;
    double mDistSq;
};
using LoopCandidateVector = std::vector<LoopCandidate>;

/* candidates -> the pairs PoseGraphOptimizerLMHIP::ComputeMarginals takes: (reference local map, query scan node) */
inline std::vector<NodePair> ToNodePairs(const LoopCandidateVector& candidates)
{
    std::vector<NodePair> pairs(candidates.size());
    for (std::size_t i = 0; i < candidates.size(); ++i)
        pairs[i] = NodePair { candidates[i].mReferenceLocalMapId, candidates[i].mQueryScanNodeId };
    return pairs;
}

/* a candidate's predicted mapLocalScanPose = InverseCompound(map pose, scan pose) (csm_host_inverse_compound):
 * the initial pose of its loop detection query and the `predicted` of LoopGate */
inline RobotPose2D<double> MapLocalScanPose(const std::array<double, 3>& localMapPose,
                                            const std::array<double, 3>& scanPose)
{
    double out[3];
    csm_host_inverse_compound(localMapPose.data(), scanPose.data(), out);
    return RobotPose2D<double> { out[0], out[1], out[2] };
}

/* LoopSearcherNearest (inc/mapping/loop_searcher_nearest.hpp:33-63) on the device (csm_loop_search). Search()
 * returns the reference's candidate set, nearest first; among equal distances at the cut, where the
 * reference's std::nth_element keeps any, the pairs with the smaller reference and then query node
 * (csm_host_loop_candidates_nearest). SearchPerMap() is the form the batch detectors want. */
class LoopSearcherNearestHIP final {
public:
    static std::unique_ptr<LoopSearcherNearestHIP> Create(double travelDistThreshold, double nodeDistThreshold,
                                                          int numOfCandidateNodes, int deviceId = 0)
    {
        if (numOfCandidateNodes < 1 || numOfCandidateNodes > CSM_LOOP_SEARCH_MAX_K)
            return nullptr;
        detail::CtxPtr ctx = detail::MakeContext(deviceId);
        if (!ctx)
            return nullptr;
        return std::unique_ptr<LoopSearcherNearestHIP>(new LoopSearcherNearestHIP(
            travelDistThreshold, nodeDistThreshold, numOfCandidateNodes, detail::ContextRef(std::move(ctx))));
    }
    /* on a context another adapter owns and keeps alive */
    LoopSearcherNearestHIP(csm_ctx* shared, double travelDistThreshold, double nodeDistThreshold,
                           int numOfCandidateNodes) :
        LoopSearcherNearestHIP(travelDistThreshold, nodeDistThreshold, numOfCandidateNodes,
                               detail::ContextRef(shared)) { }

    LoopSearcherNearestHIP(const LoopSearcherNearestHIP&) = delete;
    LoopSearcherNearestHIP& operator=(const LoopSearcherNearestHIP&) = delete;

    csm_ctx* Context() const { return this->mCtx.Get(); }
    /* pairs evaluated and eligible in the last call */
    const csm_loop_search_info& LastInfo() const { return this->mLastInfo; }

    /* LoopSearcher::Search: queries are the nodes of the last finished local map, references the nodes of
     * the maps before it, every gate measured from mAccumTravelDist */
    LoopCandidateVector Search(const LoopSearchHintView& searchHint)
    {
        const Graph g = this->ToGraph(searchHint);
        std::vector<std::int32_t> queries(g.mNumOfNodes - g.mNumOfRefs);
        std::iota(queries.begin(), queries.end(), g.mNumOfRefs);
        const std::vector<double> queryTravel(queries.size(), searchHint.mAccumTravelDist);
        std::vector<std::int32_t> counts;
        const std::vector<csm_loop_candidate> records =
            this->Run(searchHint, g, g.mNumOfRefs, queries, queryTravel, this->mNumOfCandidateNodes, false, counts);
        std::vector<csm_loop_candidate> kept(static_cast<std::size_t>(this->mNumOfCandidateNodes));
        std::int32_t numOfKept = 0;
        CSM_ASSERT_OK(this->Context(),
                      csm_host_loop_candidates_nearest(records.data(), counts.data(),
                                                       static_cast<std::int32_t>(counts.size()),
                                                       this->mNumOfCandidateNodes, this->mNumOfCandidateNodes,
                                                       kept.data(), &numOfKept));
        kept.resize(static_cast<std::size_t>(numOfKept));
        this->mLastAccumTravelDist = searchHint.mAccumTravelDist;
        this->mLast = ToCandidates(kept);
        return this->mLast;
    }

    /* Per query node the nearest reference node of each local map, the nPerQuery nearest maps
     * (one_per_map = 1). Any node up to the last finished map's last may be a reference (the local map of the
     * query itself never is), and each query's gate is measured from its own travel distance: the offline
     * search of a finished graph. Returns the used records, query by query in the order given. */
    LoopCandidateVector SearchPerMap(const LoopSearchHintView& searchHint, const std::vector<int>& queryNodes,
                                     int nPerQuery)
    {
        const Graph g = this->ToGraph(searchHint);
        std::vector<std::int32_t> queries(queryNodes.begin(), queryNodes.end());
        std::vector<double> queryTravel(queries.size());
        for (std::size_t i = 0; i < queries.size(); ++i) {
            CSM_ASSERT_THAT(queries[i] >= 0 && queries[i] < g.mNumOfNodes, "query node %d is not in the graph",
                            queries[i]);
            queryTravel[i] = g.mTravel[static_cast<std::size_t>(queries[i])];
        }
        std::vector<std::int32_t> counts;
        const std::vector<csm_loop_candidate> records =
            this->Run(searchHint, g, g.mNumOfNodes, queries, queryTravel, nPerQuery, true, counts);
        std::vector<csm_loop_candidate> used;
        for (std::size_t i = 0; i < counts.size(); ++i)
            used.insert(used.end(), records.begin() + static_cast<std::ptrdiff_t>(i) * nPerQuery,
                        records.begin() + static_cast<std::ptrdiff_t>(i) * nPerQuery + counts[i]);
        return ToCandidates(used);
    }

    /* The three value sequences the reference registers (src/mapping/loop_searcher_nearest.cpp:13-28) as it
     * observes them after a Search (:136-167), under the same ids. */
    template <typename Observe>
    void ReportMetrics(Observe&& observe) const
    {
        observe(std::string("LoopSearcherNearest.AccumTravelDist"), this->mLastAccumTravelDist);
        observe(std::string("LoopSearcherNearest.NumOfCandidateNodes"), static_cast<double>(this->mLast.size()));
        for (const LoopCandidate& c : this->mLast)
            observe(std::string("LoopSearcherNearest.NodeDist"), c.mDistSq);
    }

private:
    using Graph = detail::LoopGraph;

    LoopSearcherNearestHIP(double travelDistThreshold, double nodeDistThreshold, int numOfCandidateNodes,
                           detail::ContextRef ctx) :
        mTravelDistThreshold(travelDistThreshold), mNodeDistThreshold(nodeDistThreshold),
        mNumOfCandidateNodes(numOfCandidateNodes), mCtx(std::move(ctx)) { }

    Graph ToGraph(const LoopSearchHintView& h) const { return detail::ToLoopGraph(h, this->Context()); }

    std::vector<csm_loop_candidate> Run(const LoopSearchHintView& h, const Graph& g, std::int32_t numOfRefs,
                                        const std::vector<std::int32_t>& queries,
                                        const std::vector<double>& queryTravel, int nPerQuery, bool onePerMap,
                                        std::vector<std::int32_t>& counts)
    {
        csm_loop_search_params prm {};
        prm.travel_dist_threshold = this->mTravelDistThreshold;
        prm.node_dist_threshold = this->mNodeDistThreshold;
        prm.n_per_query = nPerQuery;
        prm.one_per_map = onePerMap ? 1 : 0;
        std::vector<csm_loop_candidate> records(queries.size() * static_cast<std::size_t>(std::max(nPerQuery, 1)));
        counts.assign(queries.size(), 0);
        CSM_ASSERT_OK(this->Context(),
                      csm_loop_search(this->Context(), h.mScanNodePoses->data(), g.mMapIndex.data(), g.mTravel.data(),
                                      g.mNumOfNodes, g.mNumOfMaps, numOfRefs, queries.data(), queryTravel.data(),
                                      static_cast<std::int32_t>(queries.size()), &prm, records.data(), counts.data(),
                                      &this->mLastInfo));
        return records;
    }

    static LoopCandidateVector ToCandidates(const std::vector<csm_loop_candidate>& records)
    {
        LoopCandidateVector out(records.size());
        for (std::size_t i = 0; i < records.size(); ++i)
            out[i] = LoopCandidate { records[i].query_scan_index, records[i].ref_scan_index,
                                     records[i].ref_map_index, records[i].dist_sq };
        return out;
    }

    const double mTravelDistThreshold, mNodeDistThreshold;
    const int mNumOfCandidateNodes;
    detail::ContextRef mCtx;
    csm_loop_search_info mLastInfo {};
    double mLastAccumTravelDist = 0.0;
    LoopCandidateVector mLast;
};

/* One scan as the descriptor build reads it: mNumOfBeams angles and ranges in the sensor's frame. */
struct ScanView {
    const double* mAngles = nullptr;
    const double* mRanges = nullptr;
    std::size_t mNumOfBeams = 0;
};

/* a LoopCandidate found by appearance, with what the descriptor comparison knows of it: the sector shift,
 * the L1 distance at that shift, the shift-free lower bound, and the heading difference theta_query -
 * theta_ref the shift implies (csm_host_descriptor_shift_angle): the centre of the matcher's theta window */
struct AppearanceCandidate {
    int mQueryScanNodeId;
    int mReferenceScanNodeId;
    int mReferenceLocalMapId;
    int mShift;
    std::uint32_t mDistance;
    std::uint32_t mRingDistance;
    double mHeadingDiff;
};
using AppearanceCandidateVector = std::vector<AppearanceCandidate>;

/* same shape as what LoopSearcherNearestHIP returns; mDistSq carries the descriptor distance */
inline LoopCandidateVector ToLoopCandidates(const AppearanceCandidateVector& candidates)
{
    LoopCandidateVector out(candidates.size());
    for (std::size_t i = 0; i < candidates.size(); ++i)
        out[i] = LoopCandidate { candidates[i].mQueryScanNodeId, candidates[i].mReferenceScanNodeId,
                                 candidates[i].mReferenceLocalMapId, static_cast<double>(candidates[i].mDistance) };
    return out;
}

/* The loop searcher by appearance (csm_scan_descriptors, csm_appearance_search), beside LoopSearcherNearestHIP
 * and on the same hint plus the scans: scans[i] is scan node i. A node's descriptor is built once, when a
 * search first sees the node, and kept; a later search builds only those of new nodes. Search() and
 * SearchPerMap() return candidates in LoopSearcherNearestHIP's shape; LastCandidates() holds the same
 * candidates with shift, distances and implied heading difference. */
class LoopSearcherAppearanceHIP final {
public:
    static std::unique_ptr<LoopSearcherAppearanceHIP> Create(double travelDistThreshold, std::uint32_t maxDistance,
                                                             int numOfCandidateNodes,
                                                             const csm_descriptor_params& descriptor,
                                                             std::uint32_t minCellSum = 0, int deviceId = 0)
    {
        if (numOfCandidateNodes < 1 || numOfCandidateNodes > CSM_LOOP_SEARCH_MAX_K)
            return nullptr;
        detail::CtxPtr ctx = detail::MakeContext(deviceId);
        if (!ctx)
            return nullptr;
        return std::unique_ptr<LoopSearcherAppearanceHIP>(new LoopSearcherAppearanceHIP(
            travelDistThreshold, maxDistance, numOfCandidateNodes, descriptor, minCellSum,
            detail::ContextRef(std::move(ctx))));
    }
    /* on a context another adapter owns and keeps alive */
    LoopSearcherAppearanceHIP(csm_ctx* shared, double travelDistThreshold, std::uint32_t maxDistance,
                              int numOfCandidateNodes, const csm_descriptor_params& descriptor,
                              std::uint32_t minCellSum = 0) :
        LoopSearcherAppearanceHIP(travelDistThreshold, maxDistance, numOfCandidateNodes, descriptor, minCellSum,
                                  detail::ContextRef(shared)) { }

    LoopSearcherAppearanceHIP(const LoopSearcherAppearanceHIP&) = delete;
    LoopSearcherAppearanceHIP& operator=(const LoopSearcherAppearanceHIP&) = delete;

    csm_ctx* Context() const { return this->mCtx.Get(); }
    const csm_loop_search_info& LastInfo() const { return this->mLastInfo; }
    const AppearanceCandidateVector& LastCandidates() const { return this->mLast; }
    /* nodes whose descriptors are kept */
    std::size_t NumOfDescriptors() const { return this->mBeamsUsed.size(); }
    void Reset()
    {
        this->mDescriptors.clear();
        this->mBeamsUsed.clear();
    }

    /* queries are the nodes of the last finished local map, references the nodes of the maps before it, every
     * gate measured from mAccumTravelDist: the numOfCandidateNodes pairs of least (distance, reference node,
     * query node) */
    LoopCandidateVector Search(const LoopSearchHintView& searchHint, const std::vector<ScanView>& scans)
    {
        const detail::LoopGraph g = detail::ToLoopGraph(searchHint, this->Context());
        std::vector<std::int32_t> queries(g.mNumOfNodes - g.mNumOfRefs);
        std::iota(queries.begin(), queries.end(), g.mNumOfRefs);
        const std::vector<double> queryTravel(queries.size(), searchHint.mAccumTravelDist);
        std::vector<csm_appearance_candidate> used =
            this->Run(g, scans, g.mNumOfRefs, queries, queryTravel, this->mNumOfCandidateNodes, false);
        std::sort(used.begin(), used.end(), [](const csm_appearance_candidate& a, const csm_appearance_candidate& b) {
            return std::tie(a.distance, a.ref_scan_index, a.query_scan_index) <
                   std::tie(b.distance, b.ref_scan_index, b.query_scan_index);
        });
        used.resize(std::min(used.size(), static_cast<std::size_t>(this->mNumOfCandidateNodes)));
        return this->Finish(used);
    }

    /* per query node the most similar reference node of each local map, the nPerQuery most similar maps
     * (one_per_map = 1); references and gates as LoopSearcherNearestHIP::SearchPerMap */
    LoopCandidateVector SearchPerMap(const LoopSearchHintView& searchHint, const std::vector<ScanView>& scans,
                                     const std::vector<int>& queryNodes, int nPerQuery)
    {
        const detail::LoopGraph g = detail::ToLoopGraph(searchHint, this->Context());
        std::vector<std::int32_t> queries(queryNodes.begin(), queryNodes.end());
        std::vector<double> queryTravel(queries.size());
        for (std::size_t i = 0; i < queries.size(); ++i) {
            CSM_ASSERT_THAT(queries[i] >= 0 && queries[i] < g.mNumOfNodes, "query node %d is not in the graph",
                            queries[i]);
            queryTravel[i] = g.mTravel[static_cast<std::size_t>(queries[i])];
        }
        return this->Finish(this->Run(g, scans, g.mNumOfNodes, queries, queryTravel, nPerQuery, true));
    }

private:
    LoopSearcherAppearanceHIP(double travelDistThreshold, std::uint32_t maxDistance, int numOfCandidateNodes,
                              const csm_descriptor_params& descriptor, std::uint32_t minCellSum,
                              detail::ContextRef ctx) :
        mTravelDistThreshold(travelDistThreshold), mMaxDistance(maxDistance), mMinCellSum(minCellSum),
        mNumOfCandidateNodes(numOfCandidateNodes), mDescriptor(descriptor), mCtx(std::move(ctx)) { }

    /* the descriptors of nodes [0, numOfNodes): those kept, and the new nodes' in one device call */
    void BuildDescriptors(const std::vector<ScanView>& scans, std::size_t numOfNodes)
    {
        const std::size_t have = this->mBeamsUsed.size();
        CSM_ASSERT_THAT(numOfNodes <= scans.size(), "a local map names a scan node whose scan is not given");
        if (numOfNodes <= have)
            return;
        std::vector<double> angles, ranges;
        std::vector<std::int32_t> offsets(1, 0);
        for (std::size_t i = have; i < numOfNodes; ++i) {
            angles.insert(angles.end(), scans[i].mAngles, scans[i].mAngles + scans[i].mNumOfBeams);
            ranges.insert(ranges.end(), scans[i].mRanges, scans[i].mRanges + scans[i].mNumOfBeams);
            offsets.push_back(static_cast<std::int32_t>(angles.size()));
        }
        if (angles.empty()) {           /* never a pointer to nothing */
            angles.push_back(0.0);
            ranges.push_back(0.0);
        }
        const std::size_t cells = static_cast<std::size_t>(this->mDescriptor.n_rings) *
                                  static_cast<std::size_t>(this->mDescriptor.n_sectors);
        this->mDescriptors.resize(numOfNodes * cells);
        this->mBeamsUsed.resize(numOfNodes);
        CSM_ASSERT_OK(this->Context(),
                      csm_scan_descriptors(this->Context(), angles.data(), ranges.data(), offsets.data(),
                                           static_cast<std::int32_t>(numOfNodes - have), &this->mDescriptor,
                                           this->mDescriptors.data() + have * cells, this->mBeamsUsed.data() + have));
    }

    /* the used records, query by query */
    std::vector<csm_appearance_candidate> Run(const detail::LoopGraph& g, const std::vector<ScanView>& scans,
                                              std::int32_t numOfRefs, const std::vector<std::int32_t>& queries,
                                              const std::vector<double>& queryTravel, int nPerQuery, bool onePerMap)
    {
        this->BuildDescriptors(scans, static_cast<std::size_t>(g.mNumOfNodes));
        csm_appearance_params prm {};
        prm.descriptor = this->mDescriptor;
        prm.travel_dist_threshold = this->mTravelDistThreshold;
        prm.max_distance = this->mMaxDistance;
        prm.min_cell_sum = this->mMinCellSum;
        prm.n_per_query = nPerQuery;
        prm.one_per_map = onePerMap ? 1 : 0;
        const std::size_t slots = static_cast<std::size_t>(std::max(nPerQuery, 1));
        std::vector<csm_appearance_candidate> records(queries.size() * slots);
        std::vector<std::int32_t> counts(queries.size(), 0);
        CSM_ASSERT_OK(this->Context(),
                      csm_appearance_search(this->Context(), this->mDescriptors.data(), g.mMapIndex.data(),
                                            g.mTravel.data(), g.mNumOfNodes, g.mNumOfMaps, numOfRefs, queries.data(),
                                            queryTravel.data(), static_cast<std::int32_t>(queries.size()), &prm,
                                            records.data(), counts.data(), &this->mLastInfo));
        std::vector<csm_appearance_candidate> used;
        for (std::size_t i = 0; i < counts.size(); ++i)
            used.insert(used.end(), records.begin() + static_cast<std::ptrdiff_t>(i * slots),
                        records.begin() + static_cast<std::ptrdiff_t>(i * slots) + counts[i]);
        return used;
    }

    LoopCandidateVector Finish(const std::vector<csm_appearance_candidate>& used)
    {
        this->mLast.resize(used.size());
        for (std::size_t i = 0; i < used.size(); ++i) {
            double heading = 0.0;
            CSM_ASSERT_OK(this->Context(),
                          csm_host_descriptor_shift_angle(used[i].shift, this->mDescriptor.n_sectors, &heading));
            this->mLast[i] = AppearanceCandidate { used[i].query_scan_index, used[i].ref_scan_index,
                                                   used[i].ref_map_index, used[i].shift, used[i].distance,
                                                   used[i].ring_distance, heading };
        }
        return ToLoopCandidates(this->mLast);
    }

    const double mTravelDistThreshold;
    const std::uint32_t mMaxDistance, mMinCellSum;
    const int mNumOfCandidateNodes;
    const csm_descriptor_params mDescriptor;
    detail::ContextRef mCtx;
    csm_loop_search_info mLastInfo {};
    std::vector<std::uint8_t> mDescriptors;
    std::vector<std::int32_t> mBeamsUsed;
    AppearanceCandidateVector mLast;
};

} /* namespace CsmHip */
#endif /* CSM_ADAPTERS_HPP */
