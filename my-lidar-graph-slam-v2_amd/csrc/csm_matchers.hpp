/* csm_matchers.hpp -- what the matchers' host translation units share (csm_plan.hip: planner, window
 * frame, job-record builders, launch helpers, levels; csm_batch.hip: batches; csm_api.hip: context, grids,
 * pyramids, host restatements, timing). csm_window.hip (one window at a time) keeps its launch chains to
 * itself: it shares nothing but its entry points of the C ABI. All of it lives in namespace csm_host. */
#ifndef CSM_MATCHERS_HPP
#define CSM_MATCHERS_HPP

#include "csm_internal.hpp"
#include "csm_joint.hpp"
#include "csm_phase.hpp"

namespace csm_host {

const int kCoarseSlices = 8;

/* score = key * kKeyToScore / n_points */
constexpr double kKeyToScore = 0.998 / (65534.0 * 499.0);

/* Launch geometry of one scoring pass (one level of one window shape). */
struct PassPlan {
    int nx = 0, ny = 0, stride = 1, log2s = 0;
    int cbx = 0, groups = 0, R = 0, ncbx = 0, ncby = 0, lstride = 0;
    bool weighted = true;     /* entries carry beam multiplicities */
    bool pairs = false;       /* pair-row fine kernel (k_score_pairs): lstride = slots per pair row */
    int lists = 1;            /* entry lists in LDS: 2 = the batch kernel that takes two slices per workgroup */
    bool joint = false;       /* ... on joint entries of the two slices (one list; csm_joint_kernels.hip) */
    bool fp32 = false;        /* this launch is the packed-fp32 bound pass of the joint kernel */
    int list_lds = -1;        /* LDS bytes of the entry lists if not lists * kPbMax words (plan_pass_pairs) */
    int ncb() const { return ncbx * ncby; }
};

/* Candidate domain and tile frame of a window (window_frame): nx x ny candidates at cell offsets
 * [x_lo, x_hi] x [y_lo, y_hi], binned over tiles_x x tiles_y tiles of the grid. */
struct WindowFrame {
    int nx = 0, ny = 0;
    int x_lo = 0, y_lo = 0, x_hi = 0, y_hi = 0;
    int tiles_x = 0, tiles_y = 0;
};

/* Launch geometry of one search window. */
struct Plan : WindowFrame {
    int n_theta = 0, n = 0;
    int win_x = 0, win_y = 0, L = 1;
    int nxc = 0, nyc = 0;
    PassPlan fine, coarse;
    int max_tiles = 0;
};

/* Work list of the exact joint kernel after the bound pass (k_bound_select): items of the main
 * launch, items of the R = 6 tail launch, their counts, workgroups to share them. */
struct JointList {
    const uint32_t* items[2] = { nullptr, nullptr };
    const uint32_t* counts = nullptr;       /* [2] */
    int blocks = 0;
};

/* Box-maximum levels to build: collected first, launched together (launch_box_jobs). */
struct PendingBox {
    DeviceGrid* grid;
    int level;          /* index into grid->levels: its cells are the destination */
};

/* The levels one call collects. A collected level reads as built (a map that a call names twice is
 * collected once) while its buffer still holds whatever hipMalloc handed out. So a list that goes
 * away before launch_box_jobs has enqueued its kernel -- an error return in between: a later map of
 * the call not resident, a window that does not fit it -- marks its levels stale: the next call that
 * wants them builds them, and csm_download_level refuses them until then. */
struct PendingBoxes {
    std::vector<PendingBox> jobs;
    bool launched = false;

    PendingBoxes() = default;
    PendingBoxes(const PendingBoxes&) = delete;
    PendingBoxes& operator=(const PendingBoxes&) = delete;
    ~PendingBoxes()
    {
        if (!launched)
            for (const PendingBox& b : jobs)
                b.grid->levels[b.level].stale = true;
    }
};

/* Splits [0, n) over up to four host threads (the batch entries touch tens of
 * megabytes of scan data before anything can be launched); fn(lo, hi) must not
 * touch the context. */
template <class F>
void host_parallel_for(int n, int grain, F fn)
{
    const int hw = (int)std::max(1u, std::thread::hardware_concurrency());
    const int nt = std::min(std::min(4, hw), n / std::max(1, grain));
    if (nt <= 1) {
        fn(0, n);
        return;
    }
    std::vector<std::thread> workers;
    for (int w = 1; w < nt; ++w)
        workers.emplace_back(fn, (int)((long)n * w / nt), (int)((long)n * (w + 1) / nt));
    fn(0, (int)((long)n / nt));
    for (auto& t : workers)
        t.join();
}

double value_to_probability(unsigned v);
int proj_theta_groups(int n_theta, long blocks_xz);
bool scan_finite_max(const csm_scan* scan, double* max_range);
void search_step_from_max(double resolution, double max_range, double* step_x, double* step_y,
                          double* step_theta);
int scans_finite_max(const csm_loop_query* queries, int n_queries, double* max_range);
bool merging_pays(const double* angles, const double* ranges, int n, double res);
int bin_hash_size(int n_points);
size_t bin_lds_bytes(int tiles, int n_points);
int ilog2_exact(int v);
bool plan_pass(const Tuning& tune, int nx, int ny, int stride, PassPlan* out);
size_t pair_lds_bytes(int ls, int cby, int lists);
bool plan_pass_pairs(const Tuning& tune, int nx, int ny, PassPlan* out, bool two_slices = false, int list_lds = -1);
int xgrid_pad_for(int nx, int ny);
int pick_buffers(const Tuning& tune, size_t lds_one, long blocks);
size_t pass_lds_bytes(const PassPlan& p);
int padded_extent(int win, int unit);
WindowFrame window_frame(const DeviceGrid& g, int win_x, int win_y, int unit);
int make_plan(csm_ctx* ctx, const DeviceGrid& g, const csm_window* w, Plan* p);
/* Job records: each starts zero-filled, with the fields every site sets the same way; the caller
 * sets the rest. */
ProjJob proj_job(const csm_geometry& geom, const double sensor_pose[3], double step_theta, int win_theta,
                 int n_points, const double* angles, const double* ranges, int32_t* hit_col, int32_t* hit_row);
BinJob bin_job(const DeviceGrid& g, const WindowFrame& f, int n_theta, int n_points, int max_tiles,
               const int32_t* hit_col, const int32_t* hit_row, uint32_t* sorted_pb, TileRec* tiles,
               int32_t* n_tiles, uint32_t* flags, int pair_mode);
ScoreJob score_job(const DeviceGrid& g, const uint16_t* cells, int stride, const BinJob& entries, int min_known);
FinalJob final_job(const ScoreJob& fine, int n_blocks, const int32_t* hit_col, const int32_t* hit_row,
                   double score_thr, const double* lut, void* out);
ExactJob exact_job(const DeviceGrid& g, const uint16_t* cells, int n_theta, int n_points, int x_lo, int y_lo,
                   int nx, int ny, int stride, const double* lut, double* out_score, uint32_t* out_k);
csm_launch::ScoreLaunch score_launch(const csm_ctx* ctx, const PassPlan& pp, dim3 grid, size_t lds);
int lane_map_for(csm_ctx* ctx, const PassPlan& pp, const uint16_t** out);
int launch_score(csm_ctx* ctx, const ScoreJob& job, const PassPlan& pp, int n_theta, int n_slices);
int launch_score_list(csm_ctx* ctx, const ScoreJob& job, const PassPlan& pp, const uint32_t* items,
                      const uint32_t* count, int blocks);
int launch_argmax(csm_ctx* ctx, const ScoreJob& job, const PassPlan& plan, int n_theta, uint32_t* sum_s,
                  uint32_t* sum_k);
bool tail_split(const csm_ctx* ctx, const PassPlan& pp);
int launch_pairs_batch(csm_ctx* ctx, const ScoreJob* jobs_dev, const PassPlan& pp, dim3 grid, BlockBase bb,
                       const JointList* list = nullptr, int which = 0);
int launch_score_batch(csm_ctx* ctx, const ScoreJob* jobs_dev, int n_jobs, const PassPlan& pp,
                       int n_theta_max, int n_slices, int theta_groups = 0, const JointList* list = nullptr);
int launch_box_jobs(csm_ctx* ctx, PendingBoxes& pending);
int build_level(csm_ctx* ctx, DeviceGrid& g, int win, Level* out);
int level_for_window(csm_ctx* ctx, DeviceGrid& g, int win, int* index,
                     PendingBoxes* pending = nullptr);
/* What a caller that names its coarse level must name: a level that is built, not stale and box-max(L). */
inline bool level_holds(const DeviceGrid& g, int level, int L)
{
    return level >= 0 && level < (int)g.levels.size() && !g.levels[level].stale && g.levels[level].win == L;
}
int ensure_xgrid(csm_ctx* ctx, DeviceGrid& g, int need_pad);
int ensure_xgrid_f(csm_ctx* ctx, DeviceGrid& g);

} /* namespace csm_host */
#endif
