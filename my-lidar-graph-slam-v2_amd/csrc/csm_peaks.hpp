/* csm_peaks.hpp -- what the units that read a window's whole score volume share: the peaks entries
 * (csm_peaks_api.hip, which defines everything declared here), the volume covariance
 * (csm_volume_api.hip) and the motion prior (csm_prior_api.hip). The device-side job record of one window,
 * the host stages of a chunk (sizing, projection on the device, exact scores + coarse known counts +
 * selection rounds), and the one host driver of the three entry shapes (volume_window, volume_batch,
 * single_query): a unit hands it a VolumeUnit -- its selection rounds, its check of a sized window, its
 * chunk body. */
#ifndef CSM_PEAKS_HPP
#define CSM_PEAKS_HPP

#include "csm_matchers.hpp"

#include <functional>

namespace csm {

constexpr int kPeakBlock = 256;      /* threads per workgroup of the selection kernels (4 wave64) */
constexpr int kPeakBlocksMax = 256;  /* workgroups per window and round: k_peaks_pick reduces one record per thread */
constexpr int kPeaksMax = CSM_PEAKS_MAX;

struct PeakJob {
    const uint32_t* s;         /* [n_theta][nx][ny] */
    const uint16_t* k;
    uint16_t* ck;              /* [n_theta][nx / L][ny / L] known counts of the coarse nodes; null: L == 1 */
    const uint16_t* cells;     /* level 0, pitched */
    const uint16_t* coarse;    /* box-max(L) level, same shape */
    int32_t rows, cols, pitch;
    const int32_t* hit_col;    /* [n_theta][n_points] */
    const int32_t* hit_row;
    const double* lut;
    const csm_result* chain;   /* the exhaustive chain's record of this window: its edge-band flag */
    csm_result* out;           /* [k_max], zero before round 0 */
    int32_t* state;            /* [0] peaks written, [1] list closed */
    BlockBest* partial;        /* [blocks] */
    int32_t n_theta, n_points, win_theta;
    int32_t nx, ny, L, x_lo, y_lo;
    int32_t min_known, blocks, chunk;   /* chunk: candidates per workgroup, blocks * chunk >= n_theta nx ny */
    int32_t k_max, excl_x, excl_y, excl_theta;
    double score_thr;
};

/* What the selection kernels of the units on these stages share (csm_peaks_kernels.hip,
 * csm_prior_kernels.hip): the f64 replay of a tie set. */

/* The reference's normalized score of candidate offsets (x, y) in slice t: the probabilities of the hit
 * cells added in beam order, one rounding per add (the 0.0 of an unknown cell adds exactly). */
__device__ __forceinline__ double replay_score(const PeakJob& job, int t, int x, int y)
{
    const int32_t* col = job.hit_col + (size_t)t * job.n_points;
    const int32_t* row = job.hit_row + (size_t)t * job.n_points;
    double sum = 0.0;
    for (int i = 0; i < job.n_points; ++i) {
        const int r = row[i] + y, c = col[i] + x;
        uint32_t v = 0;
        if (r >= 0 && r < job.rows && c >= 0 && c < job.cols)
            v = job.cells[(size_t)r * job.pitch + c];
        sum += job.lut[v];
    }
    return sum / (double)job.n_points;
}

/* (score, rank, number of candidates sharing the score): greater score first, then the smaller rank */
__device__ __forceinline__ void tie_combine(double& s, unsigned long long& r, uint32_t& same, double s2,
                                            unsigned long long r2, uint32_t same2)
{
    if (same2 == 0)
        return;
    if (same == 0 || s2 > s) {
        s = s2;
        r = r2;
        same = same2;
    } else if (s2 == s) {
        r = r2 < r ? r2 : r;
        same += same2;
    }
}

} /* namespace csm */

namespace csm_host {

constexpr int64_t kPeaksDefaultScratch = (int64_t)1 << 30;
constexpr int64_t kPeaksMaxCandidates = (int64_t)1 << 26;

/* One window of a peaks call once its arguments are checked. */
struct PeakWindow {
    uint64_t map_id = 0;
    DeviceGrid* grid = nullptr;
    csm_window w = {};
    WindowFrame f;
    int64_t total = 0;           /* candidates */
    size_t vol_bytes = 0;        /* S, K and coarse K, each padded to 256 bytes */
    size_t hit_off = 0;          /* of its hit columns in pk_hits (bytes); the rows follow */
};

/* What peaks_select_chunk leaves on the device (in ctx->pk_tab) and in pinned memory (ctx->pk_pin). */
struct PeakChunk {
    const csm::PeakJob* jobs_dev = nullptr;    /* [m] */
    const csm::PeakJob* jobs_pin = nullptr;    /* the host's copy; valid until pk_pin is written again */
    const csm_result* rec_dev = nullptr;       /* [m][k_max], followed by the states [m][2] */
    size_t back_bytes = 0;                     /* records + states */
    char* back_pin = nullptr;                  /* room for them in pk_pin */
    int n_points_max = 0;                      /* the chunk's longest scan */
};

/* The window's candidate domain and scratch need against `scratch_limit` (0: the default); nothing is
 * allocated. */
int peaks_size_window(csm_ctx* ctx, PeakWindow& pw, int64_t scratch_limit, int index);
/* The search set-up of every query as csm_correlative_match makes it (head[i]: poses, steps, window),
 * its window sized, the coarse levels built. */
int peaks_prepare_queries(csm_ctx* ctx, const csm_loop_query* queries, int n, const csm_correlative_params* prm,
                          int64_t scratch_limit, std::vector<PeakWindow>& wins, std::vector<csm_summary>& head);
/* [lo, hi) of the next chunk: windows in order while their volumes fit the limit (each fits on its own). */
int peaks_next_chunk(const std::vector<PeakWindow>& wins, int lo, int64_t scratch_limit);
/* Scans of queries [lo, hi) projected on the device into pk_hits (a window with an entry the projection
 * cannot certify: on the host); sets hit_off. Waits for the stream. */
int peaks_project_chunk(csm_ctx* ctx, const csm_loop_query* queries, std::vector<PeakWindow>& wins,
                        const std::vector<csm_summary>& head, int lo, int hi);
/* The selection of a unit: `rounds` rounds of the peaks' two launches (0: none) with these exclusion radii. */
struct PeakRounds {
    int rounds = 0, excl_x = 0, excl_y = 0, excl_theta = 0;
};
/* Windows [lo, hi) with their hit indices in pk_hits: the job table (room for max(1, sel.rounds) records
 * per window, zeroed), exact scores of every candidate, coarse known counts (peaks_score_chunk), then
 * sel.rounds selection rounds. Everything is queued on the stream; nothing is copied back and the host does
 * not wait for the selection. */
int peaks_select_chunk(csm_ctx* ctx, std::vector<PeakWindow>& wins, int lo, int hi, const PeakRounds& sel,
                       PeakChunk* out);

/* ---- the host driver of the units on the volume ---- */

/* The six entries of a symmetric 3 x 3 matrix, (kA[k], kB[k]): xx xy xt yy yt tt */
constexpr int kA[6] = { 0, 0, 0, 1, 1, 2 }, kB[6] = { 0, 1, 2, 1, 2, 2 };

/* J: MoveBackward(sensor pose, rel_pose) by the sensor pose, at a pose of heading `theta` */
inline void move_backward_jacobian(double theta, const double rel_pose[3], double J[3][3])
{
    const double sn = std::sin(theta), cs = std::cos(theta);
    const double v[3][3] = { { 1.0, 0.0, sn * rel_pose[0] + cs * rel_pose[1] },
                             { 0.0, 1.0, -cs * rel_pose[0] + sn * rel_pose[1] },
                             { 0.0, 0.0, 1.0 } };
    std::memcpy(J, v, sizeof(v));
}

/* What differs between the units. The driver sizes a window, then runs `check` (if any) on it: the unit's
 * own refusals that need the window's frame and candidate count. Per chunk it runs the stages with `sel`,
 * then `body`: the unit's own launches on the stream, and its results of windows [lo, hi) copied back into
 * the unit's own storage (which waits for the stream). Both are built once per call, not per chunk. */
struct VolumeUnit {
    PeakRounds sel;
    int64_t scratch_limit = 0;
    std::function<int(const PeakWindow& pw, int index)> check;
    std::function<int(std::vector<PeakWindow>& wins, int lo, int hi, const PeakChunk& ch)> body;
};

/* One window with the caller's hit indices and a coarse level the caller names: size, check, level, device,
 * hits into pk_hits, stages, body. A failure past the upload waits for the stream, so that no copy from the
 * caller's arrays stays pending. */
int volume_window(csm_ctx* ctx, const VolumeUnit& u, uint64_t map_id, const csm_window* w, const int32_t* hit_col,
                  const int32_t* hit_row);
/* A batch of queries: set-up (peaks_prepare_queries), check per window, then chunk by chunk projection,
 * stages, body. head[i]: the set-up's part of query i's summary. The per-query shares of the time from
 * `t0_us` (the unit's clock_us() on entry) to the first chunk and of the chunks. */
int volume_batch(csm_ctx* ctx, const VolumeUnit& u, const csm_loop_query* queries, int n,
                 const csm_correlative_params* prm, double t0_us, std::vector<csm_summary>& head, double* setup_us,
                 double* opt_us);
/* The summary of a query: the set-up's part and the timing shares; with `found`, the record and its poses. */
void fill_summary(csm_summary& o, const csm_summary& head, const csm_result& raw, bool found,
                  const double rel_pose[3], double setup_us, double opt_us);
/* The one query of a single-query entry. */
csm_loop_query single_query(uint64_t map_id, const csm_geometry* geom, const csm_scan* scan,
                            const double initial_pose[3]);

} /* namespace csm_host */
#endif
