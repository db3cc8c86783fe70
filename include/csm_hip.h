/* csm_hip.h -- C ABI of libcsm_hip.so, the MI355X (gfx950) correlative
 * scan-matching backend.
 *
 * Drop-in boundary for the correlative / branch-and-bound matching path of
 * sterngerlach/my-lidar-graph-slam-v2. Each entry point cites the reference
 * interface it replaces (paths relative to the reference tree,
 * inc/ = include/my_lidar_graph_slam/, src/ = src/my_lidar_graph_slam/).
 *
 * Conventions
 *  - plain C types only; every pointer is a host pointer unless its name ends
 *    in _dev; inputs are borrowed for the duration of the call.
 *  - every function returns 0 on success or a negative errno-style code;
 *    csm_last_error() gives the text. Nothing throws across the boundary.
 *  - one csm_ctx per matcher / detector object, single caller per ctx (the
 *    reference never shares a matcher between its two threads,
 *    src/slam_module_factory.cpp:102-104 vs src/loop_detector_factory.cpp:180-183).
 *    All mutable state lives in the ctx. The one process-wide table is a
 *    mutex-guarded record of the dynamic-LDS limit already granted to each
 *    kernel function per device (a property of the function, not of a ctx).
 *  - occupancy values are the reference's raw uint16 cells: 0 = unknown,
 *    1..65535 <-> P in [0.001, 0.999] (inc/grid_map_new/grid_binary_bayes.hpp:163-176).
 *  - there is no CPU fallback: without a GPU every compute entry point fails
 *    with CSM_ENODEV.
 *  - scans must hold finite ranges and angles ("no return" beams filtered out
 *    upstream, as the reference's scan filters do): a non-finite value makes
 *    the matching entry points fail with CSM_EINVAL.
 *  - limits: at most 10240 beams per scan (the binning kernel's tables live in LDS); LowResolution / 2^NodeHeightMax up
 *    to 64 cells; grid + window up to ~2500 x 2500 cells per map (CSM_EINVAL
 *    beyond).
 */
#ifndef CSM_HIP_H
#define CSM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSM_OK       0
#define CSM_ENOENT  (-2)   /* unknown map id / level */
#define CSM_EIO     (-5)   /* HIP runtime error */
#define CSM_ENOMEM  (-12)
#define CSM_ENODEV  (-19)  /* no usable GPU */
#define CSM_EINVAL  (-22)

/* csm_result.flags */
#define CSM_FLAG_EDGE_BAND   1u  /* a coarse read fell in the negative edge band
                                    (SURVEY 8(a) A8): resolved by the literal
                                    sequential device path */
#define CSM_FLAG_KEY_TIE     2u  /* several candidates shared the best integer
                                    key: resolved by the f64 replay */
#define CSM_FLAG_F64_TIE     4u  /* several candidates share the best f64 score
                                    bit for bit (branch-and-bound: the reference's
                                    choice then depends on heap order) */
#define CSM_FLAG_LITERAL     8u  /* result produced by the literal path */
#define CSM_FLAG_PROJ_DELTA 16u  /* branch-and-bound: some per-node projection
                                    differed from base+offset and was corrected */

typedef struct csm_ctx csm_ctx;

/* csm_config.tuning_off: switches individual launch optimisations OFF (A/B
 * measurements, parity tests of both forms). 0 = the defaults. The library never
 * reads the environment on a launch path; forced launch shapes exist only in
 * tuning builds (-DCSM_TUNING), read once in csm_create. */
#define CSM_TUNE_NO_LANE_MAP         1u   /* threads numbered through the lane groups in order */
#define CSM_TUNE_NO_XCD_MAP          2u   /* identity workgroup -> XCD order in batch launches */
#define CSM_TUNE_NO_PAIR_TAIL        4u   /* a window's last row block stays in the R = 8 launch */
#define CSM_TUNE_NO_TWO_SLICES       8u   /* batch fine kernel: one theta slice per workgroup */
#define CSM_TUNE_NO_THETA_MAJOR     16u   /* large single-window launches stay block-major */
#define CSM_TUNE_NO_TILE_SPLIT      32u   /* small single windows are never tile-split */
#define CSM_TUNE_MAP_HOST_PROJECTION 64u  /* map building: hit points computed on the host */
#define CSM_TUNE_NO_JOINT          128u   /* batch fine kernel: per-slice entry lists (round-2 form) */
#define CSM_TUNE_NO_BOUND_PASS     256u   /* no packed-fp32 bound pass: the exact integer kernel scores
                                             every candidate block */
#define CSM_TUNE_NO_TWO_PHASE      512u   /* single windows are always searched exhaustively */
#define CSM_TUNE_FORCE_TWO_PHASE  1024u   /* ... always coarse-first (default: by window size) */
#define CSM_TUNE_NO_GRAPHS        2048u   /* single queries are always launched kernel by kernel */

typedef struct {
    int32_t  device_id;          /* HIP device ordinal */
    uint32_t tuning_off;         /* CSM_TUNE_* bits */
    int32_t  map_uncertain_cap;  /* > 0: capacity of the map builder's list of uncertified
                                    beams (tests of its overflow path); 0 = default */
    int32_t  reserved[5];
} csm_config;

/* Geometry of a grid map: inc/grid_map_new/grid_map_geometry.hpp:228-240 */
typedef struct {
    double  resolution;     /* metres per cell */
    double  offset_x;       /* mPosOffset.mX */
    double  offset_y;       /* mPosOffset.mY */
} csm_geometry;

/* One scan: inc/sensor/sensor_data.hpp (ScanData<double>: Angles(), Ranges(),
 * RelativeSensorPose()) */
typedef struct {
    const double* angles;
    const double* ranges;
    int32_t       n_points;
    int32_t       reserved;
    double        relative_sensor_pose[3];
} csm_scan;

/* ScanMatcherCorrelative constructor arguments
 * (inc/mapping/scan_matcher_correlative.hpp:58-66,
 *  src/scan_matcher_factory.cpp:173-177) plus the two thresholds of the
 * 6-argument OptimizePose overload (scan_matcher_correlative.hpp:75-81) */
typedef struct {
    double  range_x, range_y, range_theta;
    int32_t low_resolution;
    int32_t reserved;
    double  score_threshold;
    double  known_rate_threshold;
} csm_correlative_params;

/* ScanMatcherBranchBound constructor arguments
 * (inc/mapping/scan_matcher_branch_bound.hpp:109-118,
 *  src/scan_matcher_factory.cpp:22-26) plus thresholds */
typedef struct {
    double  range_x, range_y, range_theta;
    int32_t node_height_max;
    int32_t reserved;
    double  score_threshold;
    double  known_rate_threshold;
} csm_bnb_params;

/* Raw search result (the device-side record; 48 bytes, also the unit of the
 * multi-GPU all-gather). Offsets are in search steps relative to the sensor
 * pose, exactly the reference's bestWinX/Y/Theta
 * (src/mapping/scan_matcher_correlative.cpp:149-152, 203-206). */
typedef struct {
    int32_t  found;
    int32_t  best_x, best_y, best_theta;
    uint64_t key;          /* 32268*K + 499*S: exact integer order of the score */
    uint32_t sum_values;   /* S: sum of raw cell values over known hit cells */
    uint32_t known;        /* K: number of known hit cells */
    uint32_t tie_count;    /* candidates sharing the best key */
    uint32_t flags;
    double   score;        /* normalized score of the winner, f64, beam order:
                              the reference's scoreMax */
} csm_result;

/* Everything ScanMatchingSummary needs from the search
 * (inc/mapping/scan_matcher.hpp:53-82) plus the metric inputs of
 * src/mapping/scan_matcher_correlative.cpp:222-236. Cost and covariance
 * (lines 209-219) stay with the caller's CostFunction. */
typedef struct {
    int32_t    pose_found;
    int32_t    win_x, win_y, win_theta;
    double     step_x, step_y, step_theta;
    double     sensor_pose[3];       /* Compound(initial, relative sensor pose) */
    double     best_sensor_pose[3];
    double     estimated_pose[3];    /* MoveBackward(best, relative sensor pose) */
    double     input_setup_us;       /* upload / pyramid time */
    double     optimization_us;
    int64_t    candidates;           /* fine candidate poses fully scored */
    csm_result raw;
} csm_summary;

/* One loop-detection query (inc/mapping/loop_detector.hpp:27-55 flattened:
 * the reference local map is named by map_id, the query scan node by scan +
 * map-local initial pose, loop_detector_branch_bound.cpp:97-104). */
typedef struct {
    uint64_t     map_id;
    csm_geometry geometry;
    csm_scan     scan;
    double       initial_pose[3];
} csm_loop_query;

/* ---- life cycle (replaces the matcher constructors; device-init failure is
 * reported like LoadBitstream does, src/slam_launcher.cpp:83-107) ---- */
int  csm_create(const csm_config* cfg, csm_ctx** out);
int  csm_destroy(csm_ctx* ctx);
const char* csm_last_error(const csm_ctx* ctx);
/* Use an existing HIP stream (hipStream_t) for all work of this ctx; NULL =
 * the ctx's own (non-blocking) stream, NOT the legacy default stream: a caller
 * that wants its work ordered with the default stream passes hipStreamLegacy /
 * hipStreamPerThread, or better a stream of its own. */
int  csm_set_stream(csm_ctx* ctx, void* hip_stream);
int  csm_synchronize(csm_ctx* ctx);

/* ---- grid maps. Replaces GridMap::CopyValues + the per-LocalMapId cache
 * (src/grid_map_new/grid_map.cpp:439-457;
 *  inc/mapping/loop_detector_branch_bound.hpp:50-69, 98;
 *  src/mapping/scan_matcher_correlative_fpga.cpp:261-262) ---- */
int  csm_upload_grid(csm_ctx* ctx, uint64_t map_id, const uint16_t* dense,
                     int32_t rows, int32_t cols);
/* The same from the reference's own storage, without the host-side flatten: GridMap<T> keeps
 * block_rows x block_cols blocks of 2^log2_block x 2^log2_block uint16, row-major inside a block,
 * each allocated or not (inc/grid_map_new/grid_map.hpp:255-263: mBlocks, mLog2BlockSize, mBlockRows,
 * mBlockCols; inc/grid_map_new/grid_binary_bayes.hpp:197-202: mValues). blocks[br * block_cols + bc]
 * points at a block's values or is NULL for an unallocated block. The library packs the allocated
 * blocks into pinned staging (one copy), de-blocks on the device into the dense level
 * GridMap::CopyValues (src/grid_map_new/grid_map.cpp:289-350, 439-457) would have produced
 * (rows = block_rows << log2_block; unallocated blocks read 0), and keeps the allocation
 * bitmap for the cost function (what csm_set_block_allocation would be given). The blocks are
 * borrowed for the duration of the call. */
int  csm_upload_grid_blocks(csm_ctx* ctx, uint64_t map_id, const uint16_t* const* blocks,
                            int32_t block_rows, int32_t block_cols, int32_t log2_block);
int  csm_has_grid(csm_ctx* ctx, uint64_t map_id);   /* 1 / 0 */
int  csm_release_grid(csm_ctx* ctx, uint64_t map_id);

/* PrecomputeGridMap(s) on device (src/mapping/grid_map_builder.cpp:987-1065):
 * level i of map_id becomes the forward box-max with window win_sizes[i]
 * (win_sizes[0] is normally 1). Level 0 always aliases the uploaded grid when
 * win_sizes[0] == 1. */
int  csm_build_pyramid(csm_ctx* ctx, uint64_t map_id, const int32_t* win_sizes,
                       int32_t n_levels);
int  csm_download_level(csm_ctx* ctx, uint64_t map_id, int32_t level,
                        uint16_t* out /* rows*cols */);
/* PrecomputeGridMaps for many finished local maps at once (what
 * LoopDetectorBranchBound::Detect does lazily per query,
 * src/mapping/loop_detector_branch_bound.cpp:83-89): makes sure every map of
 * map_ids holds box-max(win_sizes[l]) for every l, building what is missing.
 * Levels that exist are kept (unlike csm_build_pyramid, which rebuilds).
 * Asynchronous on the ctx stream. */
int  csm_build_pyramids(csm_ctx* ctx, const uint64_t* map_ids, int32_t n_maps,
                        const int32_t* win_sizes, int32_t n_levels);

/* ---- host-side set-up pieces (pure CPU, exported so the adapter and the
 * tests share one implementation) ---- */
/* ComputeSearchStep: src/mapping/scan_matcher_correlative.cpp:255-274 */
int  csm_host_search_step(double resolution, const double* ranges, int32_t n,
                          double* step_x, double* step_y, double* step_theta);
/* Window half-widths: scan_matcher_correlative.cpp:141-146 */
int  csm_host_window(double range, double step);
/* Smallest known count K with double(K)/double(n) > known_rate_threshold
 * (the test of scan_matcher_correlative.cpp:181-182 as an integer bound) */
int  csm_host_min_known(int32_t n_points, double known_rate_threshold);
/* Compound / MoveBackward: inc/pose.hpp:154-166, 215-227 */
void csm_host_compound(const double start[3], const double diff[3], double out[3]);
void csm_host_inverse_compound(const double start[3], const double end[3], double out[3]);
void csm_host_move_backward(const double end[3], const double diff[3], double out[3]);
/* ComputeScanIndices for n_theta slices t = -win_theta..win_theta
 * (scan_matcher_correlative.cpp:161-168, 277-297): out arrays are
 * [n_theta][n_points]; also returns r*cos / r*sin per slice if non-NULL
 * (needed by the branch-and-bound projection). */
int  csm_host_project(const csm_geometry* geom, const double sensor_pose[3],
                      double step_theta, int32_t win_theta,
                      const double* angles, const double* ranges, int32_t n,
                      int32_t* hit_col, int32_t* hit_row,
                      double* r_cos, double* r_sin);
/* The same projection as the matchers run it: on the device, with a
 * per-entry certificate. hit_col / hit_row [2*win_theta+1][n] (host) receive
 * the device's indices; `uncertified` receives the flat indices t*n + i of the
 * entries whose cell coordinate lies too close to a cell edge for the device's
 * sin / cos to be trusted (at most uncertified_cap of them; *n_uncertified is
 * the full count). Contract checked by the tests: every entry NOT listed
 * equals csm_host_project's (glibc) index. The matchers recompute the listed
 * ones on the host. Non-finite ranges or angles are rejected (CSM_EINVAL);
 * the reference's upstream filters drop them before the matcher sees a scan. */
int  csm_project_scan(csm_ctx* ctx, const csm_geometry* geom, const double sensor_pose[3],
                      double step_theta, int32_t win_theta,
                      const double* angles, const double* ranges, int32_t n,
                      int32_t* hit_col, int32_t* hit_row, uint32_t* uncertified,
                      int32_t uncertified_cap, int32_t* n_uncertified);
/* value -> probability table, 65536 doubles
 * (inc/grid_map_new/grid_values.hpp:26-35) */
void csm_host_probability_lut(double* lut);

/* ---- the hot path ---- */

/* Pre-projected search window, CSM flavour: replaces the theta/x/y sweep of
 * src/mapping/scan_matcher_correlative.cpp:161-197 + 339-368 for one query. */
typedef struct {
    int32_t n_theta;          /* 2*win_theta+1 */
    int32_t n_points;
    int32_t win_x, win_y;
    int32_t low_resolution;   /* L; level `coarse_level` must be box-max(L) */
    int32_t coarse_level;
    int32_t min_known;        /* csm_host_min_known() */
    int32_t merge_mode;       /* 0: merge beams that land on the same cell into
                                 weighted entries (default); 1: one entry per beam
                                 (better when beams rarely share cells) */
    double  score_threshold;
} csm_window;

/* hit_col / hit_row: [n_theta][n_points] int32, host memory. */
int  csm_score_window(csm_ctx* ctx, uint64_t map_id, const csm_window* w,
                      const int32_t* hit_col, const int32_t* hit_row,
                      csm_result* out);
/* Same with device-resident inputs and output (asynchronous on the ctx
 * stream; no host synchronisation unless a tie / edge-band path is needed,
 * in which case out_dev->flags tells and csm_resolve_window_dev() finishes). */
int  csm_score_window_dev(csm_ctx* ctx, uint64_t map_id, const csm_window* w,
                          const int32_t* hit_col_dev, const int32_t* hit_row_dev,
                          csm_result* out_dev);
/* csm_score_window_dev for n independent windows in one launch chain (the
 * batched kernels of the loop detectors): windows[i] on map_ids[i] with the
 * device-resident hit indices hit_col_dev[i] / hit_row_dev[i], result i in
 * out_dev[i] (device). Asynchronous; a record that carries a key-tie or
 * edge-band flag is finished by scoring that window again with
 * csm_score_window_dev() + csm_resolve_window_dev(). Coarse levels as for the
 * single call (csm_build_pyramid; windows[i].coarse_level). */
int  csm_score_windows_dev(csm_ctx* ctx, int32_t n, const uint64_t* map_ids,
                           const csm_window* windows, const int32_t* const* hit_col_dev,
                           const int32_t* const* hit_row_dev, csm_result* out_dev);
/* The same launch chain with dumps for parity tests of the batched kernels, each a
 * device pointer per window or NULL (per window or for a whole array):
 * dump_s_dev[i] / dump_k_dev[i]: every candidate's integer sums S [n_theta][nx][ny]
 * uint32 and K [..] uint16 (nx = ceil((2*win_x+1)/L)*L); a window with either set is
 * scored by the exact kernel on every candidate block. dump_f_dev[i]: every
 * candidate's fp32 order key from the bound pass, [n_theta][nx][ny] float (written
 * only when the bound pass runs for the window's group). */
int  csm_score_windows_dump_dev(csm_ctx* ctx, int32_t n, const uint64_t* map_ids,
                                const csm_window* windows, const int32_t* const* hit_col_dev,
                                const int32_t* const* hit_row_dev, csm_result* out_dev,
                                uint32_t* const* dump_s_dev, uint16_t* const* dump_k_dev,
                                float* const* dump_f_dev);
/* What the last single-window search (csm_correlative_match) evaluated, and whether its launch chain
 * was a replay of a recorded HIP graph (graph_replayed). Large windows are searched
 * coarse-first (scan_matcher_correlative.cpp:176-192 is the reference's pruning): every
 * coarse node is scored, then the fine level only on the candidate blocks that hold an eligible
 * coarse node reaching the best fine score found under the best coarse node. SURVEY 8(d) asks for
 * the EVALUATED poses of a pruned search next to the nominal window. */
typedef struct {
    int64_t nominal_candidates;        /* (2 win_theta + 1) * X_ext * Y_ext */
    int64_t coarse_nodes_scored;       /* 0: exhaustive search, no coarse pass needed */
    int64_t fine_candidates_scored;    /* candidates of the fine blocks scored (whole blocks) */
    int32_t two_phase;                 /* 1: coarse-first */
    int32_t graph_replayed;            /* 1: csm_correlative_match replayed a recorded graph */
    int64_t blocks_scored, blocks_skipped;
} csm_search_info;
int  csm_last_search_info(csm_ctx* ctx, csm_search_info* out);
/* Two-pass fine level of the batch entries: candidate blocks the exact
 * integer kernel scored / skipped after the packed-fp32 bound pass since the last call
 * (synchronises the context's stream; resets the counters). */
int  csm_bound_pass_stats(csm_ctx* ctx, uint64_t* blocks_scored, uint64_t* blocks_skipped);
/* Synchronises, reads *out_dev and, when it carries a key tie or an edge-band
 * flag, runs the exact device paths (f64 tie replay / literal sequential
 * sweep) for the window just scored with csm_score_window_dev(); no-op
 * otherwise. csm_score_window() does this itself. */
int  csm_resolve_window_dev(csm_ctx* ctx, uint64_t map_id, const csm_window* w,
                            const int32_t* hit_col_dev, const int32_t* hit_row_dev,
                            csm_result* out_dev);
/* Optional dump of every candidate's integer sums for parity tests:
 * S [n_theta][nx][ny] uint32 and K [..] uint16 (nx = ceil((2*win_x+1)/L)*L),
 * coarse K [n_theta][nx/L][ny/L]. Host pointers, any may be NULL. */
int  csm_score_window_dump(csm_ctx* ctx, uint64_t map_id, const csm_window* w,
                           const int32_t* hit_col, const int32_t* hit_row,
                           csm_result* out, uint32_t* dump_s, uint16_t* dump_k,
                           uint16_t* dump_coarse_k);

/* ScanMatcherCorrelative::OptimizePose, both overloads
 * (src/mapping/scan_matcher_correlative.cpp:92-115, 118-244): uploads nothing;
 * the grid must be resident under map_id; builds box-max(L) if missing. */
int  csm_correlative_match(csm_ctx* ctx, uint64_t map_id,
                           const csm_geometry* geom, const csm_scan* scan,
                           const double initial_pose[3],
                           const csm_correlative_params* params,
                           csm_summary* out);

/* LoopDetectorBranchBound::Detect's search part for a batch of queries
 * (src/mapping/loop_detector_branch_bound.cpp:59-156 lines 68-108;
 *  ScanMatcherBranchBound::OptimizePose, scan_matcher_branch_bound.cpp:111-278).
 * Every map_id must be resident; pyramids are built and cached on first use.
 * out[i] corresponds to queries[i] (pose_found = 0 when the reference would
 * `continue`). */
int  csm_bnb_match_batch(csm_ctx* ctx, const csm_loop_query* queries,
                         int32_t n_queries, const csm_bnb_params* params,
                         csm_summary* out);

/* LoopDetectorCorrelative::Detect's search part for a batch of queries
 * (src/mapping/loop_detector_correlative.cpp:59-156, lines 68-108): the
 * correlative matcher with the detector's thresholds against resident maps,
 * one coarse map (box-max L) cached per map id. out[i] <-> queries[i]. */
int  csm_correlative_match_batch(csm_ctx* ctx, const csm_loop_query* queries,
                                 int32_t n_queries, const csm_correlative_params* params,
                                 csm_summary* out);

/* ---- the K best DISTINCT poses per window (beyond the reference, which keeps scoreMax only):
 * a second peak almost as high as the first is how perceptual aliasing shows in the score volume.
 *
 * Candidates, key and eligibility are those of the single-best search: (t, x, y) over the extended
 * domain n_theta x nx x ny (nx = ceil((2 win_x + 1) / L) L), key = 32268 K + 499 S, eligible iff the
 * coarse node's known count >= min_known (L = 1: every candidate). Peak j is chosen among the eligible
 * candidates that no peak p of 0..j-1 excludes (|t - p.t| <= excl_theta and |x - p.x| <= excl_x and
 * |y - p.y| <= excl_y, in search steps, theta not wrapped): the greatest key, then the greatest f64
 * beam-order score, then the first in the reference's sweep order. The list ends at k_max, when no
 * candidate is left, or at the first peak whose score does not pass score_threshold (score > threshold,
 * as `found`). Every candidate is scored exactly (the exhaustive chain, no bound pass, no coarse-first
 * search) and the peaks are selected on the device in k_max rounds without a host round trip.
 *
 * Each record is a full csm_result: found = 1, offsets relative to the sensor pose, sum_values / known /
 * key, tie_count = remaining eligible candidates sharing the key (> 1: CSM_FLAG_KEY_TIE, resolved by the
 * f64 replay over them; CSM_FLAG_F64_TIE if several share the best f64 score too), score bit-exact.
 * Peak 0 equals the record of csm_score_window / csm_correlative_match whenever that record carries
 * neither CSM_FLAG_EDGE_BAND nor CSM_FLAG_LITERAL. For an edge-band window the peaks follow the closed
 * form above (the literal pruning path is not replayed) and every record carries CSM_FLAG_EDGE_BAND.
 * Entries past *n_peaks are zero (found / pose_found = 0).
 * CSM_EINVAL: k_max outside 1..CSM_PEAKS_MAX, a negative radius or limit, a window of more than 1 << 26
 * candidates, a single window whose score volume (6 bytes per candidate + 2 per coarse node) exceeds
 * the scratch limit. Not provided: branch-and-bound peaks, the csm_group_* entries. */
#define CSM_PEAKS_MAX 16
typedef struct {
    int32_t k_max;                       /* 1..CSM_PEAKS_MAX */
    int32_t excl_x, excl_y, excl_theta;  /* >= 0, search steps; all 0: plain top-K */
    int64_t scratch_limit_bytes;         /* 0 = default (1 GiB); batches are cut into chunks whose score
                                            volumes fit (tests force several chunks with it) */
} csm_peaks_params;

/* hit_col / hit_row as csm_score_window takes them; out[k_max]. */
int  csm_score_window_peaks(csm_ctx* ctx, uint64_t map_id, const csm_window* w,
                            const int32_t* hit_col, const int32_t* hit_row,
                            const csm_peaks_params* peaks, csm_result* out, int32_t* n_peaks);
/* csm_correlative_match's set-up; out[k_max]: best_sensor_pose / estimated_pose per peak, computed as
 * for the winner. */
int  csm_correlative_peaks(csm_ctx* ctx, uint64_t map_id, const csm_geometry* geom,
                           const csm_scan* scan, const double initial_pose[3],
                           const csm_correlative_params* params, const csm_peaks_params* peaks,
                           csm_summary* out, int32_t* n_peaks);
/* csm_correlative_match_batch's queries; out[n_queries * k_max] (query i: out[i * k_max ..]),
 * n_peaks[n_queries]. All windows of a chunk are selected together, one launch per round. */
int  csm_correlative_peaks_batch(csm_ctx* ctx, const csm_loop_query* queries, int32_t n_queries,
                                 const csm_correlative_params* params, const csm_peaks_params* peaks,
                                 csm_summary* out, int32_t* n_peaks);

/* ---- pose covariance read off the whole score volume (beyond the reference, whose only covariance is
 * the Gauss-Newton Hessian of the cost function at the winning pose): a ridge along a corridor, a plateau
 * in front of a wall, a second lobe all show in the volume and in nothing else.
 *
 * Candidates, key and eligibility are those of csm_score_window_peaks. The winner b is its peak 0 (k_max
 * = 1): the greatest key, then the greatest f64 beam-order score, then the first in sweep order; an
 * edge-band window follows the closed form and carries CSM_FLAG_EDGE_BAND, as the peaks do. If nothing is
 * eligible or the winner's score does not pass score_threshold, best.found = 0 and every moment is zero.
 *
 * Weight. With c = 0.998 / (65534 * 499) (score = key c / N, N = n_points) and tau = temperature (score
 * units): band_keys = ceil(17 tau N / c), bin_shift = the smallest s with (band_keys >> s) <
 * CSM_VOLUME_BINS, W[b] = floor(2^24 exp(-((b << bin_shift) c) / (N tau)) + 0.5) as uint32, computed on
 * the host in f64 (csm_host_volume_weights); W[0] = 2^24. An eligible candidate weighs
 * W[(key_b - key) >> bin_shift], 0 when that bin is >= CSM_VOLUME_BINS; an ineligible one weighs 0.
 *
 * Moments, exact in int64, over d = (x - x_b, y - y_b, t - t_b) in search steps (theta not wrapped):
 * m0 = sum w, m1[a] = sum w d_a, m2 = sum w d_a d_b in the order xx xy xt yy yt tt, support = candidates
 * with w > 0, border_support = those of them with x, y or t at its first or last index of the extended
 * domain (non-zero: the window truncated the distribution). Integer sums are associative, so the device
 * result equals the definition bit for bit whatever the order.
 *
 * Covariance (csm_host_volume_covariance; one fixed f64 expression, index order (x, y, theta)):
 *   num_ab = m0 m2_ab - m1_a m1_b                      exact, __int128
 *   cov_idx_ab = (double)num_ab / ((double)m0 * (double)m0)
 *   sensor_covariance_ab = (cov_idx_ab * step_a) * step_b
 *   mean_offset_a = ((double)m1_a / (double)m0) * step_a
 *   covariance = J sensor_covariance J^T, J = d MoveBackward(sensor pose, rel_pose) / d sensor pose at the
 *   estimated pose: the identity plus J[0][2] = sin(th) rx + cos(th) ry, J[1][2] = -cos(th) rx + sin(th) ry
 *   (th = estimated_pose[2], libm sin / cos). T = J S with T_ij = (J_i0 S_0j + J_i1 S_1j) + J_i2 S_2j, then
 *   covariance_ij = (T_i0 J_j0 + T_i1 J_j1) + T_i2 J_j2, every product taken (also those by 0 and 1).
 * A covariance of zeros (a support of one candidate) is a valid answer. m0 = 0 gives all zeros.
 *
 * CSM_EINVAL, all checked before anything is allocated: temperature not finite or <= 0;
 * 17 tau N / c >= 2^62; n_cand (max(n_theta, nx, ny) - 1)^2 2^24 >= 2^63; a negative scratch limit; and
 * the peaks' own refusals (more than 1 << 26 candidates, a volume beyond the scratch limit).
 * Not provided: branch-and-bound and grid-search volumes, the csm_group_* entries, a default temperature. */
#define CSM_VOLUME_BINS 1024
typedef struct {
    double  temperature;                 /* tau, in score units; finite and > 0 */
    int64_t scratch_limit_bytes;         /* as csm_peaks_params.scratch_limit_bytes */
} csm_volume_params;

typedef struct {
    csm_result best;                     /* the winner: peak 0 of csm_score_window_peaks */
    int64_t    m0, m1[3], m2[6];
    int64_t    support, border_support;
    int32_t    bin_shift, reserved;
} csm_volume_moments;

typedef struct {
    csm_summary        summary;          /* as csm_correlative_match fills it, from the winner */
    csm_volume_moments moments;
    double             mean_offset[3];           /* of the sensor pose from the winner, metric */
    double             sensor_covariance[9];     /* of the sensor pose, row-major (x, y, theta) */
    double             covariance[9];            /* of the estimated (robot) pose */
} csm_volume_summary;

/* hit_col / hit_row as csm_score_window takes them. */
int  csm_score_window_moments(csm_ctx* ctx, uint64_t map_id, const csm_window* w,
                              const int32_t* hit_col, const int32_t* hit_row,
                              const csm_volume_params* volume, csm_volume_moments* out);
/* csm_correlative_match's set-up. */
int  csm_correlative_covariance(csm_ctx* ctx, uint64_t map_id, const csm_geometry* geom,
                                const csm_scan* scan, const double initial_pose[3],
                                const csm_correlative_params* params, const csm_volume_params* volume,
                                csm_volume_summary* out);
/* csm_correlative_match_batch's queries; out[n_queries]. All windows of a chunk share each launch. */
int  csm_correlative_covariance_batch(csm_ctx* ctx, const csm_loop_query* queries, int32_t n_queries,
                                      const csm_correlative_params* params, const csm_volume_params* volume,
                                      csm_volume_summary* out);
/* Host restatements (no GPU needed). The weight table of n_points beams at `temperature`:
 * CSM_EINVAL if n_points < 1 or the temperature is refused as above. */
int  csm_host_volume_weights(int32_t n_points, double temperature, uint32_t table[CSM_VOLUME_BINS],
                             int32_t* bin_shift);
/* steps = (step_x, step_y, step_theta); estimated_pose / rel_pose as in csm_summary / csm_scan. */
int  csm_host_volume_covariance(const csm_volume_moments* moments, const double steps[3],
                                const double estimated_pose[3], const double rel_pose[3],
                                double mean_offset[3], double sensor_cov[9], double cov[9]);

/* ---- motion prior on the search window (beyond the reference, which keeps the first strict maximum in
 * sweep order: on a score plateau -- a corridor's ridge, an all-ties map -- that is the candidate nearest
 * the (-win_x, -win_y, -win_theta) corner, the pose farthest from the odometry guess the window was
 * centred on). The scan likelihood is weighed against a Gaussian prior on the offset from the initial
 * pose, as in Olson's correlative matcher.
 *
 * Candidates, key, eligibility and the extended domain are exactly those of csm_score_window_peaks. Every
 * candidate is scored exactly (no bound pass, no coarse-first search).
 *
 * Offsets. d = (x, y, t): the candidate's offset from the window centre (the sensor pose of the initial
 * guess) in search steps, the triple a csm_result carries in best_x / best_y / best_theta; theta is not
 * wrapped.
 * Prior. A symmetric 3 x 3 information matrix Lambda (row-major, index order (x, y, theta)) over the metric
 * sensor-pose offset delta = (x step_x, y step_y, t step_theta).
 * Penalised score. score - 1/2 delta^T Lambda delta, in score units. With c = 0.998 / (65534 * 499) and
 * N = n_points one score unit is N / c key units (the constant of the volume covariance above).
 * Quantisation (csm_host_motion_prior; host, f64, one fixed expression), for the six pairs in the order
 * xx xy xt yy yt tt:
 *   q_ab = ((((N / c) * m_ab) * Lambda_ab) * step_a) * step_b,   m_ab = 0.5 on the diagonal, 1.0 off it
 *   Q_ab = (int64) floor(q_ab * 256 + 0.5)
 * Penalty. pen(d) = max(0, (sum_{a<=b} Q_ab d_a d_b) >> 8): int64 arithmetic, arithmetic shift.
 * pk(d) = (int64) key - pen(d), which may be negative. Integer sums are associative, so the device equals
 * the definition whatever the order.
 * Winner. The eligible candidate with the greatest pk; among equal pk the greatest key; among those the
 * greatest f64 beam-order score (replayed over the candidates still tied, as for the peaks); among those
 * the first in the reference's sweep order. tie_count = eligible candidates sharing the winner's
 * (pk, key); CSM_FLAG_KEY_TIE / CSM_FLAG_F64_TIE as in the peaks. found = (the winner's f64 score >
 * score_threshold): the raw score is tested, not the penalised one. If nothing is eligible or the winner
 * fails the threshold, `best`, `penalty` and `penalised_key` are zeros. An edge-band window follows the
 * closed form and both records carry CSM_FLAG_EDGE_BAND, as the peaks do.
 * Result. `unweighted` is the record csm_score_window_peaks(k_max = 1) gives; both winners come out of the
 * same pass over the volume, so a caller sees how far the prior moved the answer. Lambda = 0 gives
 * best == unweighted and penalty == 0. Q is always filled.
 *
 * CSM_EINVAL, all checked before anything is allocated: a non-finite Lambda entry; an asymmetric Lambda
 * (Lambda_ab != Lambda_ba as doubles); a |q_ab * 256| that does not fit int64 (>= 2^63); 6 max|Q_ab|
 * d_max^2 >= 2^62 with d_max = max(n_theta, nx, ny) - 1; a negative scratch limit; and the peaks' own
 * refusals. A Lambda that is not positive semi-definite is allowed: the max(0, .) clamp defines the result.
 * Not provided: peaks or volume moments under a prior, branch-and-bound and grid-search, the csm_group_*
 * entries, a prior mean other than the window centre. */
typedef struct {
    double  information[9];              /* Lambda of the sensor pose, row-major (x, y, theta) */
    double  steps[3];                    /* (step_x, step_y, step_theta) of a raw window; the match entries
                                            take the steps of their search set-up and ignore these */
    int64_t scratch_limit_bytes;         /* as csm_peaks_params.scratch_limit_bytes; a batch is cut by
                                            priors[0]'s */
} csm_motion_prior;

typedef struct {
    csm_result best;                     /* the winner under the prior */
    csm_result unweighted;               /* peak 0 of csm_score_window_peaks */
    int64_t    penalty, penalised_key;   /* pen(d) and pk(d) of `best` */
    int64_t    Q[6];                     /* xx xy xt yy yt tt */
} csm_prior_result;

typedef struct {
    csm_summary      summary;            /* as csm_correlative_match fills it, from `best` */
    csm_prior_result prior;
} csm_prior_summary;

/* Host only: the quantisation and its refusals. steps = (step_x, step_y, step_theta), d_max = max(n_theta,
 * nx, ny) - 1 of the window (>= 0). */
int  csm_host_motion_prior(const double information[9], const double steps[3], int32_t n_points,
                           int32_t d_max, int64_t Q[6]);
/* Host only: the information of the sensor pose from that of the robot pose, out = J^T Lambda_robot J with
 * J = d MoveBackward(sensor pose, rel_pose) / d sensor pose at the initial pose: the identity plus
 * J[0][2] = sin(th) rx + cos(th) ry, J[1][2] = -cos(th) rx + sin(th) ry (th = initial_pose[2], libm sin /
 * cos), as for the volume covariance. T = J^T Lambda with T_ij = (J_0i L_0j + J_1i L_1j) + J_2i L_2j, then
 * out_ij = (T_i0 J_0j + T_i1 J_1j) + T_i2 J_2j for i <= j, every product taken (also those by 0 and 1);
 * out_ji = out_ij, so the result is symmetric as csm_host_motion_prior demands. rel_pose = 0 gives
 * out == robot_information for a symmetric input. */
int  csm_host_prior_from_robot_information(const double robot_information[9], const double initial_pose[3],
                                           const double rel_pose[3], double out[9]);
/* hit_col / hit_row as csm_score_window takes them. */
int  csm_score_window_prior(csm_ctx* ctx, uint64_t map_id, const csm_window* w,
                            const int32_t* hit_col, const int32_t* hit_row,
                            const csm_motion_prior* prior, csm_prior_result* out);
/* csm_correlative_match's set-up. */
int  csm_correlative_match_prior(csm_ctx* ctx, uint64_t map_id, const csm_geometry* geom,
                                 const csm_scan* scan, const double initial_pose[3],
                                 const csm_correlative_params* params, const csm_motion_prior* prior,
                                 csm_prior_summary* out);
/* csm_correlative_match_batch's queries; priors[n_queries], out[n_queries]. All windows of a chunk share
 * each launch. */
int  csm_correlative_match_prior_batch(csm_ctx* ctx, const csm_loop_query* queries, int32_t n_queries,
                                       const csm_correlative_params* params, const csm_motion_prior* priors,
                                       csm_prior_summary* out);

/* ---- likelihood-field maps (beyond the reference, which scores a scan against the raw occupancy grid):
 * every obstacle of a resident map spread by a Gaussian of the sensor's noise into a second resident map,
 * the lookup table Olson's correlative matcher scores against. The field is an ordinary uint16 grid under
 * an id of its own: every entry point that takes a map_id searches it unchanged, and the exactness of the
 * integer key and the f64 replay carries over. Cost, covariance and refinement are bilinear in occupancy
 * and belong on the source map, not on the field.
 *
 * Definition (integers only). Source grid G, rows x cols; radius R in cells, 1 <= R <=
 * CSM_LIKELIHOOD_MAX_RADIUS; threshold occupied_min >= 1; a table T[0 .. R^2] of uint32, each <= 32768,
 * indexed by the squared cell distance. A cell o is an obstacle iff it lies inside the map and G[o] >=
 * occupied_min.
 *   spread(c) = max over obstacles o with d2 = (o.r - c.r)^2 + (o.c - c.c)^2 <= R^2 of
 *                   1 + (((G[o] - 1) * T[d2]) >> 15)      (uint32: 65534 * 32768 < 2^32)
 *               0 if there is none
 *   out(c)    = G[c]                        if keep_unknown and G[c] == 0
 *               max(G[c], spread(c))        otherwise
 * With T[0] = 32768 an obstacle spreads its own value onto itself: no cell is lowered, and no value exceeds
 * the largest obstacle's (65534 at most, as in the source); a cell with no
 * obstacle within R is unchanged, so unknown stays unknown away from walls and known-rate thresholds keep
 * their meaning there. With keep_unknown = 0 an unknown cell within R of an obstacle BECOMES KNOWN (a scan
 * point that lands just behind a wall then scores the wall's likelihood instead of nothing); with
 * keep_unknown = 1 it stays 0 and only known cells are raised. An integer maximum does not depend on the
 * order of the obstacles, so the device equals csm_host_likelihood_map bit for bit.
 *
 * The table (csm_host_likelihood_kernel; host, f64, libm exp, one fixed expression; the device never
 * evaluates exp):
 *   T[d2] = (uint32) floor(32768 * exp(-(d2 * (res * res)) / (2 * (sigma * sigma))) + 0.5)
 * T[0] = 32768 and T is non-increasing. The caller passes the table in, as with the volume's weights. */
#define CSM_LIKELIHOOD_MAX_RADIUS 16
typedef struct {
    int32_t         radius;         /* R, cells: 1..CSM_LIKELIHOOD_MAX_RADIUS */
    uint32_t        occupied_min;   /* >= 1; 32768: P(occupied) above one half */
    int32_t         keep_unknown;   /* 0: unknown cells within R of an obstacle become known; else they stay 0 */
    int32_t         reserved;
    const uint32_t* kernel;         /* T: radius^2 + 1 entries, each <= 32768 */
} csm_likelihood_params;

/* Host only. ceil(3 * (sigma / resolution)) clamped to 1..CSM_LIKELIHOOD_MAX_RADIUS; CSM_EINVAL unless sigma
 * and resolution are finite and > 0. */
int  csm_host_likelihood_radius(double sigma, double resolution);
/* Host only. table[radius^2 + 1] as defined above; CSM_EINVAL for a radius out of range or a sigma or
 * resolution that is not finite and > 0. */
int  csm_host_likelihood_kernel(double sigma, double resolution, int32_t radius, uint32_t* table);
/* Host only: the definition as one plain loop over the obstacles and their taps. grid / out: dense rows x
 * cols, row-major, distinct buffers. CSM_EINVAL: rows or cols < 1, a radius out of range, occupied_min = 0,
 * no table, a table entry above 32768. */
int  csm_host_likelihood_map(const uint16_t* grid, int32_t rows, int32_t cols,
                             const csm_likelihood_params* params, uint16_t* out);
/* The field of the resident map src_map_id, built on the device into dst_map_id. Afterwards dst is in
 * exactly the state csm_upload_grid(dst, csm_host_likelihood_map(cells of src)) leaves it in: rows, cols
 * and pitch of the source, first known row / column of the new cells (counted on the device), no levels
 * above the base, the block allocation derived from the cells; an existing dst (of any shape) is replaced,
 * its cached copies dropped. src is not touched and no cell travels to the host. Returns when the field is
 * built.
 * CSM_EINVAL: dst == src, the params csm_host_likelihood_map refuses. CSM_ENOENT: src is not resident.
 * A call that is refused or fails leaves an existing dst as it was and registers nothing. */
int  csm_build_likelihood_map(csm_ctx* ctx, uint64_t src_map_id, uint64_t dst_map_id,
                              const csm_likelihood_params* params);
/* The same for n maps (src_ids[i] -> dst_ids[i]) in one launch, whatever their shapes: the fields of a
 * loop-detection batch. A source may feed several fields. CSM_EINVAL also when a dst appears twice or is
 * one of the sources; nothing is built then. */
int  csm_build_likelihood_maps(csm_ctx* ctx, const uint64_t* src_ids, const uint64_t* dst_ids, int32_t n,
                               const csm_likelihood_params* params);

/* ---- distance fields (beyond the reference): every cell's squared distance to its NEAREST obstacle, exact
 * over the whole map, and a second resident map read off it through a caller's table. Where the likelihood
 * field above visits every obstacle within R of a cell (so R <= 16), a distance transform costs the same at
 * any radius: a field that decays over metres for global searches, the distance sensor model (the probability
 * of a beam as a function of the distance from its end point to the nearest obstacle), clearance masks,
 * chamfer scores, nearest-obstacle correspondences. The field is an ordinary uint16 grid under an id of its
 * own, as the likelihood field is.
 *
 * Definition (integers only). Source grid G, rows x cols (pad columns are not cells), both at most 32767;
 * threshold occupied_min >= 1. A cell o is an obstacle iff it lies inside the map and G[o] >= occupied_min.
 *   d2(c)      = min over obstacles o of (o.r - c.r)^2 + (o.c - c.c)^2      (uint32)
 *                CSM_DISTANCE_NONE if the map has no obstacle
 *   nearest(c) = o.r * cols + o.c of the obstacle that attains d2(c); among several the smallest such index
 *                (smallest row, then smallest column); CSM_DISTANCE_NONE if there is none
 *   out(c)     = 0                        if keep_unknown and G[c] == 0
 *                T[min(d2(c), R^2)]       otherwise
 * T[0 .. R^2]: the caller's table of uint16, each <= 65534, R in 1..CSM_DISTANCE_MAX_RADIUS. T[R^2] is what
 * every cell farther than R from all obstacles gets: 0 leaves them unknown, a positive floor makes the whole
 * map known. d2 and nearest are NOT capped by R. Squared distances are integers and a minimum does not depend
 * on the order it is taken in, so device, host function and definition agree in every bit. A ramp, a
 * truncated quadratic (1 + min(d2, cap), whose sum over a scan's end points is the chamfer score) or a hard
 * clearance mask are tables like any other.
 *
 * The usual table (csm_host_distance_kernel; host, f64, libm exp, one fixed expression; the device never
 * evaluates exp):
 *   T[d2] = floor_value + (uint16) floor((peak - floor_value) * exp(-(d2 * (res * res)) / (2 * (sigma * sigma))) + 0.5) */
#define CSM_DISTANCE_MAX_RADIUS 255
#define CSM_DISTANCE_NONE       0xFFFFFFFFu
/* device scratch of one launch chain of csm_build_distance_maps (2 bytes per cell): a batch beyond it is cut
 * into chunks of maps, a single map beyond it runs alone (the convention of csm_host_map_batch_plan) */
#define CSM_DISTANCE_SCRATCH_LIMIT (1ll << 30)
typedef struct {
    int32_t         radius;         /* R, cells: 1..CSM_DISTANCE_MAX_RADIUS */
    uint32_t        occupied_min;   /* >= 1; 32768: P(occupied) above one half */
    int32_t         keep_unknown;   /* 0: every cell gets its table entry; else unknown cells of the source stay 0 */
    int32_t         reserved;
    const uint16_t* table;          /* T: radius^2 + 1 entries, each <= 65534 */
} csm_distance_params;

/* Host only. table[radius^2 + 1] as defined above; CSM_EINVAL for a radius out of range, a sigma or resolution
 * that is not finite and > 0, or unless floor_value <= peak <= 65534. */
int  csm_host_distance_kernel(double sigma, double resolution, int32_t radius, uint32_t peak,
                              uint32_t floor_value, uint16_t* table);
/* Host only: d2 and nearest of a dense rows x cols grid, row-major; either output may be null. A plain
 * sequential restatement of the device's two passes (column offsets, then per cell a walk over the columns
 * that hold an obstacle). CSM_EINVAL: rows or cols < 1 or > 32767, occupied_min = 0, both outputs null. */
int  csm_host_distance_transform(const uint16_t* grid, int32_t rows, int32_t cols, uint32_t occupied_min,
                                 uint32_t* d2, uint32_t* nearest);
/* Host only: out(c) of the definition. grid / out: dense rows x cols, distinct buffers. CSM_EINVAL: what
 * csm_host_distance_transform refuses, a radius out of range, no table, a table entry above 65534. */
int  csm_host_distance_map(const uint16_t* grid, int32_t rows, int32_t cols,
                           const csm_distance_params* params, uint16_t* out);
/* d2 and nearest of the resident map map_id, computed on the device and copied to the host buffers (dense
 * rows x cols each; either may be null, not both). The map, its levels and its derived copies are not
 * touched. Runs on the ctx stream and returns when the outputs are written. CSM_EINVAL: occupied_min = 0,
 * both outputs null, a map with more than 32767 rows or columns. CSM_ENOENT: the map is not resident. */
int  csm_distance_transform(csm_ctx* ctx, uint64_t map_id, uint32_t occupied_min, uint32_t* d2,
                            uint32_t* nearest);
/* The field of the resident map src_map_id, built on the device into dst_map_id. Afterwards dst is in
 * exactly the state csm_upload_grid(dst, csm_host_distance_map(cells of src)) leaves it in, on the terms of
 * csm_build_likelihood_map: shape of the source, first known row / column counted on the device, no levels
 * above the base, derived copies stale, block allocation derived from the cells, base_epoch bumped when the
 * id existed. src is not touched and no cell travels to the host. Returns when the field is built.
 * CSM_EINVAL: dst == src, the params csm_host_distance_map refuses, a source with more than 32767 rows or
 * columns. CSM_ENOENT: src is not resident. A call that is refused or fails leaves an existing dst as it was
 * and registers nothing. */
int  csm_build_distance_map(csm_ctx* ctx, uint64_t src_map_id, uint64_t dst_map_id,
                            const csm_distance_params* params);
/* The same for n maps (src_ids[i] -> dst_ids[i]) of any shapes on one launch chain (two kernels; chunks of
 * maps beyond CSM_DISTANCE_SCRATCH_LIMIT). A source may feed several fields. CSM_EINVAL also when a dst
 * appears twice or is one of the sources; nothing is built then. */
int  csm_build_distance_maps(csm_ctx* ctx, const uint64_t* src_ids, const uint64_t* dst_ids, int32_t n,
                             const csm_distance_params* params);

/* ---- free-space check of loop candidates (beyond the reference, whose detectors accept a pose on the
 * score of the scan's END POINTS alone): every beam of a scan walked from the sensor to its hit, as the map
 * builder would walk it if it integrated the scan at this pose, and the cells it crosses classified against
 * the resident map. A pose on the wrong side of a wall scores like the true one; only its rays run through
 * cells the map knows to be occupied. Read-only: the map is never resized or written.
 *
 * Definition (integers only once the hit points are formed). A query's initial_pose is the map-local ROBOT
 * pose to check (a summary's estimated_pose).
 *   S = Compound(initial_pose, relative_sensor_pose)                         (csm_host_compound)
 *   scaledRes = res / subpixel_scale                                         (ScaledGeometry, as the builder)
 *   sX = floor((S.x - offX) / scaledRes), sY likewise
 * Beam i is USABLE iff r > usable_range_min && r < usable_range_max (a NaN range is unusable; for finite r
 * the builder's rule, grid_map_builder.cpp:618-619). For a usable beam
 *   h  = (S.x + r cos(S.theta + a), S.y + r sin(S.theta + a))                (ScanData::HitPoint)
 *   H  = (floor((h.x - offX) / res), floor((h.y - offY) / res))              the hit cell
 *   (eX, eY) = the same expression at scaledRes                              the sub-pixel end
 *   W  = the cells of BresenhamScaled(sX, sY, eX, eY) (src/bresenham.cpp:58-237) with its / and % read as
 *        floored division and its remainder. Where the reference is defined (it asserts non-negative
 *        coordinates) that is its own walk; elsewhere it is the same ray moved by whole cells: with
 *        b = (floor_div(min(sX, eX), scale), floor_div(min(sY, eY), scale)), W = b + the reference's walk
 *        of the ray moved by -b * scale, which is non-negative. A move by whole cells changes no
 *        remainder, so it moves the cells and nothing else. No walk holds a cell twice.
 *   E  = (floor_div(eX, scale), floor_div(eY, scale)); the MISSED cells M are W without E
 *        (grid_map_builder.cpp:904-910).
 * Only cells inside rows x cols of level 0 of the resident map are read and counted. A cell c of M inside
 * the map, with value v and depth d = max(|c.x - H.x|, |c.y - H.y|), is
 *   unknown   v == 0
 *   free      0 < v <= free_max
 *   blocking  v >= occupied_min and d >  end_tolerance
 *   near      v >= occupied_min and d <= end_tolerance      (the wall the beam ends on is some cells thick)
 *   other     anything else
 * A usable beam is WALKED iff it has a missed cell inside the map or H lies inside; BLOCKED iff it has a
 * blocking cell. If H lies inside, its value v puts the beam in end_unknown (v == 0), end_free (0 < v <=
 * free_max), end_occupied (v >= occupied_min) or none of them. Every count is an integer and integer sums do
 * not depend on the order, so the device equals csm_host_ray_check field for field (host_beams aside).
 *
 * 64 bits. CSM_EINVAL keeps |S - off| / res <= 2^20 per axis, usable_range_max / res <= 2^20 and
 * subpixel_scale <= CSM_RAY_CHECK_MAX_SCALE = 512, so every sub-pixel coordinate lies within (2^21 + 2) * 512
 * < 2^31 of zero. After the move by -b * scale the four coordinates lie in [0, 2^30). Then, in the closed
 * form of csm_map.hpp (dx = eX - sX etc.): den = 2 scale dx < 2^40; y0 < 2^21, so n0 = y0 den + (2 (sY %
 * scale) + 1) dx < 2^61 + 2^40; first + 2 scale j + last < 2^31 + 2^11 (j <= 2^21), so |dy| (..) < 2^61 +
 * 2^41; and n0 + dy (..) + den < 2^62 + 2^42 < 2^63. */
#define CSM_RAY_CHECK_MAX_SCALE 512
typedef struct {
    double   usable_range_min, usable_range_max;
    int32_t  subpixel_scale;        /* 1..CSM_RAY_CHECK_MAX_SCALE; the builder's is 100 */
    int32_t  end_tolerance;         /* cells, >= 0 */
    uint32_t occupied_min, free_max;   /* raw cell values, 0 < free_max < occupied_min <= 65535 */
    int64_t  scratch_limit_bytes;   /* 0 = default (1 GiB). A batch is cut into chunks of consecutive queries: a
                                       query of n beams counts 36 n + 256 bytes, and a chunk is closed before
                                       the query that would take it past the limit (a query that alone
                                       exceeds it gets a chunk of its own) */
} csm_ray_check_params;

typedef struct {
    int32_t beams;                  /* n_points */
    int32_t usable, walked, blocked;
    int32_t end_inside, end_occupied, end_free, end_unknown;
    int64_t cells;                  /* missed cells inside the map, all classes */
    int64_t cells_free, cells_unknown, cells_near, cells_blocking;
    int32_t max_depth;              /* greatest depth of a blocking cell, 0 if there is none */
    int32_t host_beams;             /* diagnostic, not part of the definition: beams whose hit point the host
                                       recomputed with glibc (csm_host_ray_check: 0) */
} csm_ray_check_result;

/* Host only. occupied_min = the smallest value 1..65535 whose probability (csm_host_probability_lut) is >=
 * prob_occupied; free_max = the greatest whose probability is <= prob_free. CSM_EINVAL: a null pointer, a
 * probability that is not finite, no such value, or free_max >= occupied_min. */
int  csm_host_ray_check_values(double prob_occupied, double prob_free, uint32_t* occupied_min, uint32_t* free_max);
/* Host only: the definition as a sequential restatement on a dense rows x cols grid (row-major, as
 * csm_upload_grid takes it), every ray walked step by step (not by the closed form). `pose` is the robot
 * pose (a query's initial_pose). per_beam (may be NULL): scan->n_points words, per beam -2 unusable, -1
 * usable but not walked, 0 walked and not blocked, otherwise that beam's greatest blocking depth.
 * CSM_EINVAL: null pointers (per_beam aside), rows or cols < 1, n_points < 0, a resolution that is not
 * finite and > 0, thresholds out of order (0 < free_max < occupied_min <= 65535), subpixel_scale outside
 * 1..CSM_RAY_CHECK_MAX_SCALE, a negative end_tolerance or scratch_limit_bytes, usable ranges that are NaN, a
 * non-finite pose, offset or angle, a sensor position more than 2^20 cells from the map's origin on an
 * axis, usable_range_max / res > 2^20. */
int  csm_host_ray_check(const uint16_t* grid, int32_t rows, int32_t cols, const csm_geometry* geom,
                        const csm_scan* scan, const double pose[3], const csm_ray_check_params* params,
                        csm_ray_check_result* result, int32_t* per_beam);
/* The check of every query against its resident map, on the device: results[i] <-> queries[i]; per_beam
 * (may be NULL) receives the queries' words back to back in query order (sum of n_points entries). One
 * launch chain per chunk of queries: all beams projected in one launch under the map builder's certificate
 * (the few uncertifiable beams recomputed with glibc on the host and patched in; more of them than the
 * context's map_uncertain_cap, or CSM_TUNE_MAP_HOST_PROJECTION, and the hit points of that chunk and of the
 * rest of the call all come from the host), one wavefront per ray over the closed form of its cells, one
 * read-back of records and words. Scans that queries of a chunk share by pointer are staged once.
 * CSM_EINVAL (before anything runs): what csm_host_ray_check refuses, for any query; n_queries < 1.
 * CSM_ENOENT: a map that is not resident. Nothing on the context changes either way. */
int  csm_ray_check_batch(csm_ctx* ctx, const csm_loop_query* queries, int32_t n_queries,
                         const csm_ray_check_params* params, csm_ray_check_result* results, int32_t* per_beam);

/* ---- pose sets: one scan scored at many free poses (the device form of ScoreFunction::Score,
 * ScorePixelAccurate::Score, score_function_pixel_accurate.cpp:16-58), and the measurement update of a
 * particle set on top of it. Every other scoring entry walks a regular window of whole search steps around
 * one pose; here every pose is an arbitrary map-local SENSOR pose (relative_sensor_pose is not applied).
 *
 * Record of pose p. Its hit cells are those csm_host_project returns for sensor pose p with win_theta = 0
 * (glibc, arg = theta + a_i, floor((h - off) / res)). S = the sum of the raw values of the hit cells that lie
 * inside the map and are known (value != 0), K = their count: what csm_score_window reads at offset (0, 0).
 * The order key is 32268 K + 499 S, as everywhere else. flags: 0, or CSM_POSE_UNCERTAIN |
 * CSM_POSE_HOST_PROJECTED for a pose the device could not certify (below); csm_host_score_poses writes 0.
 *
 * Device. The cosine and sine of every beam angle are taken once per scan and those of theta once per pose;
 * cos / sin(theta + a_i) come from the addition theorems, and an index counts only if floor() cannot flip
 * within the error bound of the matchers' projection (two library calls, two products, one sum: 2.4e-15 +
 * 4e-16 (|theta| + |a_i|) on the cosine, x64 margin on the quotient). A pose with any beam inside that
 * margin of a cell edge is marked CSM_POSE_UNCERTAIN; after one read-back of their count the host projects
 * exactly those poses with glibc and a second kernel scores them from the host's indices
 * (CSM_POSE_HOST_PROJECTED). All sets of a call share each launch; sets that pass the same angles / ranges
 * pointers and n_points stage the scan once.
 *
 * CSM_EINVAL, checked before anything is allocated: null pointers, n_sets < 0, n_poses < 0, n_points < 1, a
 * non-finite pose, angle, range, offset or a resolution that is not finite and > 0, a pose
 * whose cell coordinate could reach 2^30 in magnitude ((|x - off_x| + max |r|) / res >= 2^30, y alike),
 * n_points > 65536 (65536 values of at most 65535 keep S within 32 bits, 0xFFFF0000 at the most, and the key
 * below 2^42), 2^30 or more poses in one call, 2^30 or more beams of distinct scans in one call. Ranges may be
 * zero or negative. n_sets = 0 and n_poses = 0 are valid and launch nothing.
 * CSM_ENOENT, checked as early: a map_id that is not resident (as every other entry reports it). */
#define CSM_POSE_UNCERTAIN       1u   /* a beam within the certificate's margin of a cell edge */
#define CSM_POSE_HOST_PROJECTED  2u   /* scored again from indices the host computed with glibc */
#define CSM_POSE_SET_MAX_POSES   (1 << 18)   /* csm_pose_set_update: poses and outputs per call */
typedef struct {
    uint64_t      map_id;        /* any resident map: occupancy, likelihood field */
    csm_geometry  geometry;
    csm_scan      scan;          /* relative_sensor_pose is NOT applied: poses are sensor poses */
    const double* poses;         /* [n_poses][3], map-local sensor poses */
    int32_t       n_poses, reserved;
} csm_pose_set;
typedef struct { uint32_t sum_values, known, flags, reserved; } csm_pose_record;   /* S, K */
typedef struct {
    int64_t poses;               /* scored in this call */
    int32_t uncertain_poses;     /* marked CSM_POSE_UNCERTAIN by the device */
    int32_t changed_poses;       /* of them: records whose S or K differ after the rescore */
    double  host_us;             /* glibc projection of the uncertain poses */
    double  device_us;           /* first launch to last, HIP events on the ctx stream */
} csm_pose_sets_info;
/* out: the records of all sets, concatenated in set order. info may be NULL. */
int  csm_score_pose_sets(csm_ctx* ctx, const csm_pose_set* sets, int32_t n_sets,
                         csm_pose_record* out, csm_pose_sets_info* info);
/* Host restatement on a dense row-major grid (no GPU needed); the same refusals. */
int  csm_host_score_poses(const uint16_t* grid, int32_t rows, int32_t cols, const csm_geometry* geom,
                          const csm_scan* scan, const double* poses, int32_t n_poses, csm_pose_record* out);
/* One fixed f64 expression: score = ((double)(32268 K + 499 S) * c) / (double)n_points with c = 0.998 /
 * (65534 * 499) as above (volume covariance), known_rate = (double)K / (double)n_points. It is not the
 * beam-order sum: it lies within 1e-12 of ScorePixelAccurate's normalised score for n_points <= 1080 (N
 * additions of terms <= 1 round by at most about N^2 2^-53 on the sum, 1.2e-13 after the division).
 * CSM_EINVAL: n_points < 1 or a null pointer. */
int  csm_host_score_from_sums(uint32_t sum_values, uint32_t known, int32_t n_points, double* score,
                              double* known_rate);

/* Measurement update of a pose set: integer weights and systematic resampling, exact integer arithmetic
 * after the scoring, so the device equals csm_host_pose_set_update bit for bit.
 *   eligible_i  K_i >= csm_host_min_known(n_points, known_rate_threshold)
 *   key_max     the greatest key over eligible poses; best_index the first pose that has it
 *   w_i         W[(key_max - key_i) >> bin_shift], W and bin_shift from csm_host_volume_weights(n_points,
 *               temperature); 0 when that bin is >= CSM_VOLUME_BINS and for an ineligible pose
 *   m0          sum w_i (u64); support = poses with w_i > 0
 *   ancestors   C_i = the inclusive prefix sum of w in pose order, u = offset mod m0,
 *               T_j = (j m0 + u) / n_out (integer division), ancestors[j] = the smallest i with C_i > T_j
 * No eligible pose: found = 0, best_index = -1, key_max = m0 = support = 0, every weight 0, every ancestor -1.
 * bin_shift is always the table's. Device chain behind the scoring and its rescore, no read-back between:
 * keys, maximum, weights and their prefix sums (one workgroup, wavefront scans), one binary search per output.
 * CSM_EINVAL: n_poses or n_out above CSM_POSE_SET_MAX_POSES (j m0 + u stays below 2^61), n_out < 0, a
 * temperature csm_host_volume_weights refuses, a known_rate_threshold that is NaN, and what
 * csm_score_pose_sets refuses. records [n_poses], weights [n_poses], ancestors [n_out]; weights and
 * ancestors may be NULL (n_poses = 0, n_out = 0). */
typedef struct { double temperature; double known_rate_threshold; int32_t n_out, reserved; uint64_t offset; } csm_pose_update_params;
typedef struct { uint64_t m0; uint64_t key_max; int32_t best_index, support, bin_shift, found; } csm_pose_update_info;
int  csm_pose_set_update(csm_ctx* ctx, const csm_pose_set* set, const csm_pose_update_params* params,
                         csm_pose_record* records, uint32_t* weights, int32_t* ancestors,
                         csm_pose_update_info* update, csm_pose_sets_info* info);
int  csm_host_pose_set_update(const csm_pose_record* records, int32_t n_poses, int32_t n_points,
                              const csm_pose_update_params* params, uint32_t* weights, int32_t* ancestors,
                              csm_pose_update_info* update);

/* ---- virtual scans: beams cast through a resident map (beyond the reference, which only ever walks a
 * MEASURED beam). From a sensor pose, in a direction: which is the first cell of the map that stops the beam,
 * and how far is it? Read-only. The sets are csm_pose_set, read as follows: `poses` are map-local SENSOR poses
 * (relative_sensor_pose is not applied), scan.angles[n_points] are the beam angles, scan.ranges is NULL or
 * holds a limit per beam.
 *
 * Definition (integers only once the end points are formed), for pose p and beam i:
 *   limit  range_max if scan.ranges == NULL. Otherwise the beam is CAST iff r_i > 0 (a NaN is not cast), with
 *          limit = r_i < range_max ? r_i : range_max.
 *   s, e, W  exactly the ray check's objects (above) for a beam of range `limit` from sensor pose p:
 *          s = floor((p.xy - off) / scaledRes), e = ScanData::HitPoint's double expression at scaledRes, W the
 *          cells of BresenhamScaled(s, e) under the floored reading, after the whole-cell move.
 *   order  The sensor's cell floor_div(s, scale) is one end of W (no walk holds a cell twice). W is read from
 *          that end: the reference's order when it did not swap its end points, the reverse when it did. (A
 *          walk is a sequence of columns with a run of rows each, both monotone; the reference starts at the
 *          cell of the end point with the smaller x, or for one column at the smaller row; the other end point
 *          lies in the last cell.)
 *   dist   For a cell c, D = 2 c scale + scale - 2 s - 1 per axis (twice the distance, in sub-pixels, from the
 *          centre of the sensor's sub-pixel to the centre of the cell), dist2 = Dx^2 + Dy^2 as int64.
 *   stop   min_dist2 = m^2, m = csm_host_ray_cast_min_dist2's (below). Walk W in order. Cells outside rows x
 *          cols of level 0 and cells with dist2 < min_dist2 are passed over. The first remaining cell with
 *          value v >= occupied_min stops the ray, kind CSM_CAST_OCCUPIED; with unknown_stops so does the first
 *          with v == 0, kind CSM_CAST_UNKNOWN. E = floor_div(e, scale) is part of W and can be the stop.
 *   record cell, value, kind, dist2 of the stop; all zero (CSM_CAST_NONE) for a beam that is not cast or does
 *          not stop. Records are pose-major per set ([n_poses][n_points]), sets concatenated.
 * The device writes no floating-point result: it equals csm_host_ray_cast record for record.
 *
 * 64 bits. The ray check's limits hold here (|p - off| / res <= 2^20 per axis, range_max / res <= 2^20,
 * subpixel_scale <= CSM_RAY_CHECK_MAX_SCALE), so the closed form stays within 2^63 as shown there. A cell of W
 * lies between s and e per axis, up to one cell: |D| <= 2 |e - s| + 2 scale <= 2 (2^20 + 1) 512 + 2^10 < 2^30.1,
 * and dist2 < 2^61.2 < 2^62. m is capped at 2^31, so min_dist2 <= 2^62 fits and then no cell stops a ray. */
#define CSM_CAST_NONE      0
#define CSM_CAST_OCCUPIED  1
#define CSM_CAST_UNKNOWN   2
typedef struct {
    double   range_max, range_min;  /* range_max finite and > 0; range_min >= 0 (may be +inf: nothing stops) */
    int32_t  subpixel_scale;        /* 1..CSM_RAY_CHECK_MAX_SCALE; the builder's is 100 */
    uint32_t occupied_min;          /* raw cell value, 1..65535 */
    int32_t  unknown_stops;         /* 0 | 1 */
    int32_t  reserved;              /* 0 */
    int64_t  scratch_limit_bytes;   /* 0 = default (1 GiB). A call is cut into chunks of consecutive poses (a
                                       chunk may end inside a set): a pose of n beams counts 48 n + 64 bytes (ray
                                       record, result record, workgroup counters, its share of the scan, pose
                                       entry), and a chunk is closed before the pose that would take it past the
                                       limit (a pose that alone exceeds it gets a chunk of its own) */
} csm_ray_cast_params;
typedef struct {
    int32_t  cell_x, cell_y;        /* the stopping cell (column, row) */
    uint32_t value;                 /* its raw value */
    int32_t  kind;                  /* CSM_CAST_* */
    int64_t  dist2;
} csm_ray_cast_record;
typedef struct {
    int64_t rays;                   /* records written */
    int64_t host_rays;              /* diagnostic, not part of the records: rays whose end point the host
                                       recomputed with glibc */
    int64_t cells_read;             /* cells of level 0 the walk loaded: whole groups of up to 64 per ray */
    int64_t cells_to_stop;          /* cells inside the map up to and including each ray's stop (all of them
                                       for a ray that does not stop); cells_read / cells_to_stop is the price of
                                       one ray per wavefront */
    double  host_us;                /* glibc end points */
    double  device_us;              /* first launch to last, HIP events on the ctx stream */
} csm_ray_cast_info;

/* Host only: m = (int64)ceil(2 range_min / (resolution / subpixel_scale)), at most 2^31; *min_dist2 = m^2.
 * CSM_EINVAL: a null pointer, range_min NaN or negative, a resolution that is not finite and > 0,
 * subpixel_scale outside 1..CSM_RAY_CHECK_MAX_SCALE. */
int  csm_host_ray_cast_min_dist2(double range_min, double resolution, int32_t subpixel_scale, int64_t* min_dist2);
/* Host only: ranges[k] = (0.5 * (resolution / subpixel_scale)) * sqrt((double)records[k].dist2) for a record
 * that stopped, none_value otherwise. One fixed f64 expression. CSM_EINVAL: null pointers (n > 0), n < 0, a
 * resolution that is not finite and > 0, subpixel_scale outside 1..CSM_RAY_CHECK_MAX_SCALE. */
int  csm_host_ray_cast_ranges(const csm_ray_cast_record* records, int64_t n, double resolution,
                              int32_t subpixel_scale, double none_value, double* ranges);
/* Host only: the definition as a sequential restatement on a dense rows x cols grid (row-major), every ray
 * walked step by step (not by the closed form). records [n_poses][scan->n_points].
 * CSM_EINVAL: null pointers (scan->ranges aside; angles, poses and records only where there is something to
 * read or write), rows or cols < 1, n_points < 0, n_poses < 0, a resolution that is not finite and > 0,
 * subpixel_scale outside 1..CSM_RAY_CHECK_MAX_SCALE, occupied_min outside 1..65535, unknown_stops other than
 * 0 | 1, a negative scratch_limit_bytes, range_max not finite or <= 0, range_min NaN or negative, a non-finite
 * pose, offset or angle, a sensor position more than 2^20 cells from the map's origin on an axis,
 * range_max / res > 2^20. */
int  csm_host_ray_cast(const uint16_t* grid, int32_t rows, int32_t cols, const csm_geometry* geom,
                       const csm_scan* scan, const double* poses, int32_t n_poses,
                       const csm_ray_cast_params* params, csm_ray_cast_record* records);
/* The cast of every set against its resident map, on the device. One launch chain per chunk of poses: all end
 * points in one launch under the map builder's certificate at the sub-pixel resolution (the few uncertifiable
 * rays recomputed with glibc on the host and patched in; more of them than the context's map_uncertain_cap, or
 * CSM_TUNE_MAP_HOST_PROJECTION, and the end points of that chunk and of the rest of the call all come from the
 * host), one wavefront per ray over the closed form of its cells from the sensor's end, which stops reading at
 * the ray's stop; one read-back of the records. Scans that sets of a chunk share by pointer are staged once.
 * info may be NULL. n_sets = 0, n_poses = 0 and n_points = 0 are valid and launch nothing.
 * CSM_EINVAL (before anything runs): what csm_host_ray_cast refuses, for any set; n_sets < 0; 2^30 or more
 * poses in one set. CSM_ENOENT: a map that is not resident. The call reads the map only and keeps nothing on
 * the context but workspaces. */
int  csm_ray_cast(csm_ctx* ctx, const csm_pose_set* sets, int32_t n_sets, const csm_ray_cast_params* params,
                  csm_ray_cast_record* records, csm_ray_cast_info* info);

/* The raw records (csm_summary.raw) of the last csm_bnb_match_batch /
 * csm_correlative_match_batch call on this ctx, in query order, copied device
 * to device into dst_dev[n_queries] on the ctx stream (asynchronous): the
 * send buffer of the multi-GPU all-gather without a host round trip
 * (the concatenation of src/mapping/loop_detector_fpga_parallel.cpp:53-56). */
int  csm_copy_last_batch_records(csm_ctx* ctx, csm_result* dst_dev);

/* ---- the step after every search: cost, covariance, sub-cell refinement ----
 * CostSquareError (inc/mapping/cost_function_square_error.hpp;
 * src/mapping/cost_function_square_error.cpp:48-195, 232-341: bilinear
 * interpolation of the four nearest cells, squared error to 1, Gauss-Newton
 * Hessian, covariance = Hessian^-1 * CovarianceScale) and
 * ScanMatcherLinearSolver::OptimizePose
 * (src/mapping/scan_matcher_linear_solver.cpp:66-169: damped Gauss-Newton
 * steps, lambda halved / doubled between 1e-8 and 1e-4), which every matcher
 * and loop detector runs on the pose the search returns
 * (scan_matcher_correlative.cpp:209-219, loop_detector_branch_bound.cpp:123-127).
 * Batched: one launch for all queries of a Detect() call.
 *
 * TOLERANCE (f64, not bit-exact): hit points come from the device's sin / cos,
 * sums over the beams are tree reductions, and Eigen's 3x3 inverse / column-
 * pivoting QR are restated from their algorithms. Against the reference's
 * arithmetic: costs and Hessian entries agree to 1e-10 relative; covariance
 * entries to 1e-8 relative to the largest entry; a refined pose to 1e-7 (m,
 * rad) when both sides run the same number of iterations -- the count can
 * differ when |cost change| lies within 1e-10 of ConvergenceThreshold, or when
 * a hit point sits within ~1e-12 cells of a cell edge (the bilinear value is
 * continuous there, its gradient is not). The tests compare at these bounds.
 *
 * Map reads are GridMap::ProbabilityOr(row, col, 0.5)
 * (src/grid_map_new/grid_map.cpp:423-436): 0.5 outside the map or in a block
 * that was never allocated, the cell's probability (0 for unknown) otherwise.
 * Allocation is not part of the dense export; the library keeps it per map
 * (rules beside csm_set_block_allocation). */
typedef struct {
    double  covariance_scale;       /* CostSquareError: "CovarianceScale" */
    int32_t iterations_max;         /* "NumOfIterationsMax" */
    int32_t reserved;
    double  convergence_threshold;  /* "ConvergenceThreshold" */
    double  lambda;                 /* the solver object's damping factor when the call starts
                                       ("InitialLambda" on its first call); every query of a batch
                                       starts from it (the reference carries it from query to query:
                                       a change of <= 1e-4 on diagonals of 1e2 and more) */
} csm_refine_params;

typedef struct {
    double  normalized_initial_cost;   /* Cost(start) / n_points */
    double  normalized_cost;           /* Cost(final) / n_points: ScanMatchingSummary::mNormalizedCost */
    double  sensor_pose[3];            /* where the evaluation started */
    double  best_sensor_pose[3];
    double  estimated_pose[3];         /* MoveBackward(best sensor pose, relative sensor pose) */
    double  covariance[9];             /* row-major, map-local: mEstimatedCovariance */
    double  hessian[9];                /* at the final pose, undamped */
    double  lambda;                    /* damping factor after the call */
    int32_t iterations;
    int32_t reserved;
} csm_refine_result;

/* allocated: one byte per block (non-zero = allocated), row-major
 * [ceil(rows / 2^log2)][ceil(cols / 2^log2)]: GridMap::IsAllocated of any cell
 * of the block. Null: the rule "a block is allocated iff it holds a known
 * cell" on blocks of 2^log2 cells (log2 0: every cell its own block).
 *
 * Each map carries the reference's allocation state:
 *  - csm_upload_grid: the rule, on 16-cell blocks ("PatchSize" 16). Exact for
 *    maps that were only ever updated (every update leaves a value >= 1 and
 *    allocates its block, grid_map.cpp:514-535, 645-700).
 *  - csm_upload_grid_blocks: its blocks; a NULL block is unallocated.
 *  - csm_set_block_allocation: as given, until the map changes.
 *  - csm_construct_map_from_scans, csm_update_map_with_scan: the old map's
 *    blocks moved by the block shift of Resize / Expand (the ones outside the
 *    new map dropped; ResetValues keeps them allocated, grid_map.cpp:278-287,
 *    841-936), plus every block a cell update touched, on blocks of
 *    shape->log2_block_size. The old map is the resident map_id if its rows
 *    and cols are shape's: its bitmap if that is on shape's blocks, else the
 *    rule on them. If map_id is not resident or its rows or cols differ,
 *    nothing was allocated (a fresh GridMap). */
int  csm_set_block_allocation(csm_ctx* ctx, uint64_t map_id, int32_t log2_block_size,
                              const uint8_t* allocated);
/* Cost / n and ComputeCovariance at sensor_poses[i] (3 doubles per query: the
 * best sensor pose of the search), scan and map of queries[i] (initial_pose is
 * not read). */
int  csm_cost_covariance_batch(csm_ctx* ctx, const csm_loop_query* queries, int32_t n_queries,
                               const double* sensor_poses, double covariance_scale,
                               csm_refine_result* out);
/* ScanMatcherLinearSolver::OptimizePose for every query: queries[i].initial_pose
 * is the map-local ROBOT pose to refine (the search's mEstimatedPose). */
int  csm_linear_solver_batch(csm_ctx* ctx, const csm_loop_query* queries, int32_t n_queries,
                             const csm_refine_params* params, csm_refine_result* out);

/* ---- the other cost type and the hill-climbing matcher ----
 * CostGreedyEndpoint (inc/mapping/cost_function_greedy_endpoint.hpp;
 * src/mapping/cost_function_greedy_endpoint.cpp: Cost, ComputeGradient,
 * ComputeCovariance) and ScanMatcherHillClimbing::OptimizePose
 * (src/mapping/scan_matcher_hill_climbing.cpp:72-180), the "GreedyEndpoint" /
 * "HillClimbing" keys of src/cost_function_factory.cpp:11-30 and
 * src/scan_matcher_factory.cpp:103-130.
 *
 * EXACT (bit-identical, unlike the square-error tolerance above): per beam the
 * cost depends only on the integer cells of the hit and missed points
 * (ScanData::HitAndMissedPoint, inc/sensor/sensor_data.hpp:252-273) and on a
 * table lookup; map reads are ProbabilityOr(row, col, 0.0), so "outside the
 * map", "unallocated block" and "unknown cell" all read 0 and are skipped (no
 * allocation bitmap is needed). Every result equals the reference's
 * arithmetic bit for bit: the sums are the literal beam-order double sums
 * whenever a comparison is not decided with margin by a bounded approximation
 * (DESIGN.md 4d), and a query any of whose hit or missed coordinates lies too
 * close to a cell edge for the device's sin / cos to be trusted is finished by
 * the host restatement below (result.host_path = 1). */
#define CSM_TUNE_GREEDY_LITERAL_SUMS 4096u  /* every hill-climbing decision from the literal sums */

#define CSM_GREEDY_KERNEL_SIZE_MAX 8     /* KernelSize 0..8 */

/* CostGreedyEndpoint constructor arguments (cost_function_factory.cpp:17-22) */
typedef struct {
    double  map_resolution;       /* "MapResolution": the cost table's cell size (not the grid's) */
    double  hit_and_missed_dist;  /* "HitAndMissedDist" */
    double  occupancy_threshold;  /* "OccupancyThreshold" */
    int32_t kernel_size;          /* "KernelSize", 0..CSM_GREEDY_KERNEL_SIZE_MAX */
    int32_t reserved;
    double  standard_deviation;   /* "StandardDeviation" (> 0) */
    double  scaling_factor;       /* "ScalingFactor" */
} csm_greedy_params;

/* ScanMatcherHillClimbing constructor arguments (scan_matcher_factory.cpp:113-116) */
typedef struct {
    double            linear_step;      /* "LinearStep" (> 0) */
    double            angular_step;     /* "AngularStep" (> 0) */
    int32_t           max_iterations;   /* "MaxIterations" (>= 1) */
    int32_t           max_refinements;  /* "MaxNumOfRefinements" */
    csm_greedy_params cost;             /* "CostConfigGroup" */
} csm_hill_climbing_params;

typedef struct {
    double  normalized_initial_cost;   /* Cost(start) / n_points: the InitialCost metric */
    double  normalized_cost;           /* Cost(best) / n_points: ScanMatchingSummary::mNormalizedCost */
    double  sensor_pose[3];            /* Compound(initial, relative sensor pose) */
    double  best_sensor_pose[3];
    double  estimated_pose[3];         /* MoveBackward(best sensor pose, relative sensor pose) */
    double  covariance[9];             /* row-major, map-local: mEstimatedCovariance */
    double  diff_translation;          /* metrics: Distance(initial, estimated) */
    double  diff_rotation;             /*          |initial.theta - estimated.theta| */
    int32_t iterations;                /* NumOfIterations */
    int32_t refinements;               /* NumOfRefinements */
    int32_t replays;                   /* passes whose decisions took the literal sums */
    int32_t host_path;                 /* 1: finished by the host restatement */
    int64_t cost_evaluations;          /* Cost() calls, covariance included */
} csm_hill_climbing_result;

/* CostGreedyEndpoint::Cost / n and ComputeCovariance at sensor_poses[i] (3
 * doubles per query: the search's best sensor pose), scan and map of
 * queries[i] (initial_pose is not read): the GreedyEndpoint counterpart of
 * csm_cost_covariance_batch. out[i]: normalized_initial_cost ==
 * normalized_cost, sensor_pose == best_sensor_pose == sensor_poses[i],
 * estimated_pose, covariance; iterations = refinements = 0. */
int  csm_greedy_cost_covariance_batch(csm_ctx* ctx, const csm_loop_query* queries, int32_t n_queries,
                                      const double* sensor_poses, const csm_greedy_params* params,
                                      csm_hill_climbing_result* out);
/* ScanMatcherHillClimbing::OptimizePose for every query: queries[i].initial_pose
 * is the map-local ROBOT pose (as in csm_linear_solver_batch). One launch chain
 * for the whole batch; n_queries = 1 is the frontend's call. */
int  csm_hill_climbing_batch(csm_ctx* ctx, const csm_loop_query* queries, int32_t n_queries,
                             const csm_hill_climbing_params* params, csm_hill_climbing_result* out);
/* Host restatements (pure CPU, glibc): the fallback of the two entries above and
 * the CPU-testable reference for the device. grid: dense rows x cols raw cells
 * (row-major, as csm_upload_grid takes them). csm_host_greedy_cost: *cost =
 * Cost() (ScalingFactor applied, not normalized); covariance (may be NULL) =
 * ComputeCovariance() at the same pose. */
int  csm_host_greedy_cost(const uint16_t* grid, int32_t rows, int32_t cols, const csm_geometry* geom,
                          const csm_scan* scan, const double sensor_pose[3],
                          const csm_greedy_params* params, double* cost, double* covariance);
int  csm_host_hill_climbing(const uint16_t* grid, int32_t rows, int32_t cols, const csm_geometry* geom,
                            const csm_scan* scan, const double initial_pose[3],
                            const csm_hill_climbing_params* params, csm_hill_climbing_result* out);

/* ---- several GPUs behind one detector object, in one process ----
 * The reference's precedent is LoopDetectorFPGAParallel
 * (src/mapping/loop_detector_fpga_parallel.cpp:42-56): Detect() cuts the query
 * vector into contiguous halves, runs one std::thread per FPGA core and
 * concatenates the per-core results. A csm_group owns one csm_ctx per listed
 * device; its batch calls cut the queries into contiguous blocks
 * (csm_shard_bounds), run one host thread per member on its block and finish
 * with ONE exchange of the 48-byte best records (csm_allgather_results). */
typedef struct csm_group csm_group;

/* Block [*lo, *hi) of `member`: sizes differ by at most one, earlier members
 * take the larger blocks (n_members = 2: the first half / second half split of
 * loop_detector_fpga_parallel.cpp:42-46). Pure host arithmetic. */
void csm_shard_bounds(int32_t n_queries, int32_t member, int32_t n_members,
                      int32_t* lo, int32_t* hi);
/* One context per entry of device_ids (CSM_ENODEV if one cannot be opened,
 * like LoadBitstream's failure, src/slam_launcher.cpp:83-107). Listing a
 * device twice gives two members on it (two streams): meant for tests on a
 * one-GPU box. */
int  csm_group_create(const int32_t* device_ids, int32_t n_devices, csm_group** out);
/* The same with the members' configuration (member_cfg->device_id is ignored; NULL =
 * defaults) and CSM_GROUP_* flags. */
#define CSM_GROUP_FORCE_RCCL 1u  /* take the RCCL exchange also for a single member (a one-rank
                                    communicator: the call sequence on a one-GPU box) */
int  csm_group_create_ex(const int32_t* device_ids, int32_t n_devices, const csm_config* member_cfg,
                         uint32_t flags, csm_group** out);
int  csm_group_destroy(csm_group* group);
int32_t csm_group_size(const csm_group* group);
/* The member's context: upload / release the maps of the queries its block will
 * hold through it (csm_upload_grid, csm_has_grid, ...). Owned by the group. */
csm_ctx* csm_group_member(csm_group* group, int32_t member);
const char* csm_group_last_error(const csm_group* group);

/* csm_bnb_match_batch / csm_correlative_match_batch over the group: queries
 * [lo_k, hi_k) go to member k, whose context must hold their maps; out[i] <->
 * queries[i]. Ends with csm_allgather_results; out[i].raw is the record that
 * came back through the exchange. */
int  csm_group_bnb_match_batch(csm_group* group, const csm_loop_query* queries, int32_t n_queries,
                               const csm_bnb_params* params, csm_summary* out);
int  csm_group_correlative_match_batch(csm_group* group, const csm_loop_query* queries,
                                       int32_t n_queries, const csm_correlative_params* params,
                                       csm_summary* out);
/* The exchange step of the last group batch (where the reference concatenates
 * two vectors, src/mapping/loop_detector_fpga_parallel.cpp:53-56): every
 * member's block of device-resident records, padded to the largest block, is
 * all-gathered so that EVERY member's device buffer holds all records.
 * Members on distinct devices: ncclAllGather (RCCL over xGMI; librccl is
 * loaded on first use). One member, or members sharing a device: copies
 * through the host. host_out (may be null) receives the n_queries records in
 * query order, read back from member 0's gathered buffer. */
int  csm_allgather_results(csm_group* group, csm_result* host_out);
/* Member `member`'s gathered device buffer after csm_allgather_results:
 * n_members blocks of *block records each (block k = member k's queries, the
 * tail of a shorter block zero). Valid until the next group batch. */
int  csm_group_gathered_records_dev(csm_group* group, int32_t member,
                                    const csm_result** dev, int32_t* block);
/* used_rccl: 1 if the exchange runs over RCCL; last_gather_us: host wall time
 * of the last csm_allgather_results. */
int  csm_group_exchange_info(const csm_group* group, int32_t* used_rccl, double* last_gather_us);

/* ScanMatcherGridSearch constructor arguments + thresholds
 * (inc/mapping/scan_matcher_grid_search.hpp, src/scan_matcher_factory.cpp) */
typedef struct {
    double range_x, range_y, range_theta;
    double step_x, step_y, step_theta;
    double score_threshold;
    double known_rate_threshold;
} csm_grid_search_params;

/* ScanMatcherGridSearch::OptimizePose, both overloads
 * (src/mapping/scan_matcher_grid_search.cpp:69-190): brute force over
 * accumulated-double offsets, every pose projected on its own
 * (ScorePixelAccurate::Score), a pose counts only if its own known rate passes.
 * In the summary win_x / win_y / win_theta hold the number of x / y / theta
 * offsets and raw.best_x / best_y / best_theta the winner's loop indices
 * (-1 when nothing was found). */
int  csm_grid_search_match(csm_ctx* ctx, uint64_t map_id, const csm_geometry* geom,
                           const csm_scan* scan, const double initial_pose[3],
                           const csm_grid_search_params* params, csm_summary* out);

/* ---- map building: the producer of the matcher's input ---- */

/* One scan node of the window [scanNodeIdMin, scanNodeIdMax]
 * (ScanNode, inc/mapping/pose_graph.hpp; ScanData, inc/sensor/sensor_data.hpp) */
typedef struct {
    double   global_pose[3];      /* ScanNode::mGlobalPose */
    csm_scan scan;
    double   min_range, max_range;   /* ScanData::MinRange / MaxRange */
} csm_scan_node;

/* GridMapBuilder constructor arguments that the map update reads
 * (src/mapping/grid_map_builder.cpp:68-99) + its SubpixelScale constant
 * (inc/mapping/grid_map_builder.hpp:294) */
typedef struct {
    double  usable_range_min, usable_range_max;
    double  prob_hit, prob_miss;
    int32_t subpixel_scale;
} csm_map_builder_params;

/* GridMapGeometry + block size of a GridMap (inc/grid_map_new/grid_map.hpp).
 * In: the map BEFORE the call (Resize works in its frame). Out: after it. */
typedef struct {
    double  resolution, offset_x, offset_y;
    int32_t rows, cols;
    int32_t log2_block_size;
} csm_map_shape;

typedef struct {
    int64_t rays;               /* usable beams integrated */
    int64_t cell_updates;       /* hit + miss updates applied */
    int64_t saturated_reads;    /* updates of a cell already at 65535: the reference's odds table
                                   (grid_values.cpp:74-77) has no such entry (undefined behaviour
                                   there); this library extends the table's formula */
    int32_t first_known_row, first_known_col;
    int32_t device_projection;  /* 1: hit points computed on the device under a certificate (the few
                                   uncertifiable beams redone with glibc); 0: all on the host */
    int32_t reserved;
    double  host_us;            /* poses, projection round trip, resize */
    double  device_us;          /* upload + kernels of the update */
} csm_map_build_info;

/* Host only. GridMap<T>::Resize(BoundingBox<int>) (src/grid_map_new/grid_map.cpp:841-889)
 * on `shape`: box = { min col, min row, max col, max row } (inclusive cell
 * indices in the map's current frame), blocks per IndexToBlock (:804-814),
 * offsets per GridMapGeometry::Resize (grid_map_geometry.cpp:61-72). With
 * expand != 0 GridMap<T>::Expand (:915-936) runs first: nothing changes if the
 * box fits, else it is joined with the current extent. shift_out (may be null)
 * = first row, first column of the new map in the old frame. */
int  csm_host_map_resize(csm_map_shape* shape, const int32_t box[4], int32_t expand,
                         int32_t shift_out[2]);

/* GridMapBuilder::ConstructMapFromScans (src/mapping/grid_map_builder.cpp:561-695)
 * = UpdateLatestMap's work (:497-527): bounding box of the sensor positions and
 * usable hit points, GridMap::Resize + ResetValues, then a sub-pixel ray cast
 * per beam (BresenhamScaled, src/bresenham.cpp:58-237) with binary-Bayes miss /
 * hit updates in beam order. The finished map becomes (or replaces) the
 * resident grid `map_id`, ready for the matchers; csm_download_level(level 0)
 * returns it as CopyValues would. `info` may be null. */
int  csm_construct_map_from_scans(csm_ctx* ctx, uint64_t map_id, csm_map_shape* shape,
                                  const double global_map_pose[3], const csm_scan_node* nodes,
                                  int32_t n_nodes, const csm_map_builder_params* params,
                                  csm_map_build_info* info);

/* The grid half of GridMapBuilder::UpdateGridMap
 * (src/mapping/grid_map_builder.cpp:389-494): one new scan into the local map
 * that is being built. The bounding box starts at the sensor position
 * (ComputeBoundingBoxAndScanPointsMapLocal, :820-872); GridMap::Expand
 * (grid_map.cpp:915-961) leaves the map alone if the box fits and otherwise
 * resizes it to the union with its current extent, keeping the cells; then the
 * same ray casts as above on top of the existing values. `map_id` must be
 * resident (uploaded, or built by these calls) with the rows / cols of `shape`. */
int  csm_update_map_with_scan(csm_ctx* ctx, uint64_t map_id, csm_map_shape* shape,
                              const double global_map_pose[3], const csm_scan_node* node,
                              const csm_map_builder_params* params, csm_map_build_info* info);

/* ---- many maps per call ----
 * What GridMapBuilder::AfterLoopClosure announces ("Re-create the local grid maps and latest map after
 * the loop closure", grid_map_builder.cpp:134) and does not do: after an optimization every local map
 * is re-cast from its moved scan nodes. Also AppendLocalMap's first build and offline mapping. */

/* One map of csm_construct_maps_from_scans: the arguments of csm_construct_map_from_scans. */
typedef struct {
    uint64_t             map_id;
    csm_map_shape        shape;              /* in: the map before the call; out: after (as the single call) */
    double               global_map_pose[3];
    const csm_scan_node* nodes;
    int32_t              n_nodes;
    int32_t              status;             /* out: CSM_OK or what the single call would have returned */
    csm_map_build_info   info;               /* out: per map; host_us / device_us are the chunk's, divided
                                                evenly among its maps: rough shares. The chunk's host_us
                                                runs from its start to the first launch of the update
                                                chain, so it holds the wait for the projection's
                                                read-back and for the uploads of patched rays */
} csm_map_build_job;

typedef struct {
    int64_t scratch_limit_bytes;   /* 0 = default (1 GiB), as csm_peaks_params.scratch_limit_bytes */
} csm_map_batch_params;

typedef struct {
    int32_t chunks;                /* launch chains the call was cut into */
    int32_t host_projection_jobs;  /* jobs whose hit points all came from the host path */
    int64_t scan_bytes_uploaded;   /* angles + ranges actually copied (shared scans counted once) */
    double  host_us, device_us;
} csm_map_batch_info;

/* csm_construct_map_from_scans for every job, with each step of the build launched once per chunk of
 * jobs instead of once per job, and two read-backs per chunk (bounding boxes and uncertain-beam counts
 * after the projection; counters at the end) instead of two per map. Afterwards the context holds what
 * a loop of the single call over the jobs, in order and not stopping at a failing job, leaves: shapes,
 * cells (byte-equal), first known row / column, block allocation, stale levels, dropped phase-major and
 * pair-row copies, and each job's info counters.
 *  - A job the single call refuses (no nodes, a node without a scan, a bad shape, an empty bounding
 *    box, a resize out of range, more than 2^24 beams) leaves its map alone; a job whose rays leave
 *    the resized map has its map dropped. Its status says so, the other jobs complete, and the call
 *    returns the first status in job order that is not CSM_OK.
 *  - CSM_EINVAL before anything changes: a null ctx / jobs / params, n_jobs < 1, bad params (as the
 *    single call), a negative scratch_limit_bytes, or the same map_id in two jobs.
 *  - params holds for all jobs (one pair of update tables); everything else is per job.
 *  - Chunks: consecutive jobs, cut by csm_host_map_batch_plan. Before the projection a map's cell
 *    count is not known; the entry plans with the bound (2 R + extent of the sensor positions + 2 res)
 *    / res + 2 + 2 blocks per axis, R = the largest usable range of the job's nodes, capped at the
 *    2^28 cells a map may have. The buffers themselves are sized by what the resize gives.
 *  - Scans: each distinct (angles, ranges, n_points) of a chunk is staged and uploaded once.
 *  - A map with more uncertain beams than the context's cap, or whose certified beams are not known to
 *    spread, takes the host projection on its own; the rest of its chunk stays on the device.
 * Limit: the hits of one cell are ranked by brute force (quadratic in the hits per cell), as in the
 * single call: a global map of thousands of scans in one job is slow here. That map is
 * csm_construct_global_map's (below), which sorts long hit lists. `batch` and `info` may be null.
 * A device or allocation failure (CSM_EIO, CSM_ENOMEM) ends the call: the jobs not yet finished get
 * that status, their maps may have been dropped, and `info` holds what had run. */
int  csm_construct_maps_from_scans(csm_ctx* ctx, csm_map_build_job* jobs, int32_t n_jobs,
                                   const csm_map_builder_params* params, const csm_map_batch_params* batch,
                                   csm_map_batch_info* info);

/* Host only, no GPU: the cut of csm_construct_maps_from_scans. Job j has n_beams[j] beams and at most
 * n_cells_upper[j] cells; its scratch is n (24 + 16) bytes of rays and records (n = max(n_beams, 1)),
 * 4 * ((11 n_beams + 23) & ~3) bytes of lists, 12 bytes per cell and 8 * 135 bytes of counters. Jobs
 * are taken in order; a chunk is closed before the job that would take it past scratch_limit_bytes
 * (0 = 1 GiB), so a job that alone exceeds the limit gets a chunk of its own. chunk_of[n_jobs]: the
 * chunk of each job; chunk_bytes[n_jobs]: the first *n_chunks entries hold the chunks' scratch.
 * CSM_EINVAL: null pointers, n_jobs < 1, a negative limit, an n_beams[j] outside 0 .. 2^24 or an
 * n_cells_upper[j] outside 0 .. 2^28 (what one map build may have). */
int  csm_host_map_batch_plan(const int64_t* n_beams, const int64_t* n_cells_upper, int32_t n_jobs,
                             int64_t scratch_limit_bytes, int32_t* chunk_of, int64_t* chunk_bytes,
                             int32_t* n_chunks);

/* ---- one map of many scans: the global map ----
 * LidarGraphSlam::GetGlobalMap -> GridMapBuilder::ConstructGlobalMap (grid_map_builder.cpp:162-184):
 * ConstructMapFromScans over every scan node of the pose graph, in the frame of the first node. */

typedef struct {
    int64_t scratch_limit_bytes;  /* 0 = default (1 GiB), as csm_map_batch_params */
    int32_t rank_direct_max;      /* 0 = default (32). A cell with at most this many hits is ranked as in the
                                     single call (each hit counts the earlier arrivals); longer lists are sorted */
    int32_t rank_tile;            /* 0 = default (4096). Entries one workgroup sorts in LDS at a time; a power of
                                     two >= 4 and <= 16384 (64 KB of LDS). Lists longer than this are sorted tile
                                     by tile and ranked across tiles */
} csm_global_map_params;

typedef struct {
    int32_t parts;                /* launch chains the build was cut into */
    int32_t max_hits_per_cell;    /* largest hit list of any part */
    int64_t direct_cells, sorted_cells, tiled_cells;   /* hit cells by rank path, summed over parts */
    int64_t beams;                /* all beams of all nodes: may exceed 2^24 */
    double  host_us, device_us;
} csm_global_map_info;

/* GridMapBuilder::ConstructGlobalMap (grid_map_builder.cpp:162-184). Leaves exactly what
 * csm_construct_map_from_scans with the same arguments leaves -- the cells of level 0 byte for byte,
 * `shape`, first known row / column, block allocation, stale levels, dropped phase-major and pair-row
 * copies, and info's rays, cell_updates and saturated_reads -- for any scratch_limit_bytes,
 * rank_direct_max and rank_tile, without that call's two limits:
 *  - The hits of a cell are ranked by a sort once there are more than rank_direct_max of them (the
 *    single call counts, for every hit, all hits of its cell: quadratic in the revisits).
 *  - The nodes are cut in order into parts (csm_host_global_map_parts on the beams of the nodes and the
 *    cells of the resized map) that are cast one after the other onto the same cells: a cell's value
 *    depends only on its own sequence of hits and misses in ray order, and the parts' sequences
 *    concatenate. The limit of 2^24 beams holds per part, so per node here; the scratch is one part's.
 *    The bounding box comes from a pass over all nodes before the one resize; with more than one part
 *    the hit points are computed again when their part is cast.
 * Refusals and the dropped map (a ray leaves the resized map) are the single call's; the cap of 2^28
 * cells per map stays. CSM_EINVAL before anything changes: a negative scratch_limit_bytes or
 * rank_direct_max, a rank_tile that is not a power of two in 4 .. 16384. `global`, `info` and
 * `global_info` may be null. info->device_projection is 1 if every part was projected on the device.
 * scratch_limit_bytes bounds what the planner counts (rays, records, lists, per-cell words, counters),
 * not all memory of a part: the entry also stages a part's angles and ranges on the device (16 bytes per
 * beam of the largest part) and on the host, and a part projected on the host holds its rays there once.
 * host_us (both infos): the host steps up to the first launch of the cast phase, plus, when the parts are
 * projected again, each part's projection with its read-back and patches; device_us: the span of the cast
 * phase between two events, less that. */
int  csm_construct_global_map(csm_ctx* ctx, uint64_t map_id, csm_map_shape* shape,
                              const double global_map_pose[3], const csm_scan_node* nodes, int32_t n_nodes,
                              const csm_map_builder_params* params, const csm_global_map_params* global,
                              csm_map_build_info* info, csm_global_map_info* global_info);

/* Host only, no GPU: the cut of csm_construct_global_map. Node k has n_beams[k] beams, the resized map
 * n_cells cells. Parts are runs of consecutive nodes, in order. A part's scratch is what
 * csm_host_map_batch_plan counts for ONE job with the part's beams and n_cells cells (the per-cell words
 * of the whole map are cleared and used again by every part). A part is closed before the node that
 * would take it past scratch_limit_bytes (0 = 1 GiB) or past 2^24 beams; a node that alone exceeds the
 * limit gets a part of its own. part_of[n_nodes]: the part of each node; part_bytes[n_nodes]: the first
 * *n_parts entries hold the parts' scratch. CSM_EINVAL: null pointers, n_nodes < 1, a negative limit,
 * an n_beams[k] outside 0 .. 2^24 or n_cells outside 0 .. 2^28. */
int  csm_host_global_map_parts(const int64_t* n_beams, int32_t n_nodes, int64_t n_cells,
                               int64_t scratch_limit_bytes, int32_t* part_of, int64_t* part_bytes,
                               int32_t* n_parts);

/* Host only. The scan-node poses of GridMapBuilder::ConstructMapFromAllScans (grid_map_builder.cpp:
 * 698-817, declared and never called): out_global_poses[i] = Compound(local_map_pose, local_poses[i])
 * (LocalMapNode::mGlobalPose, ScanNode::mLocalPose; csm_host_compound), n triples each. A caller fills
 * csm_scan_node.global_pose with them, nodes in ascending id, and calls csm_construct_global_map. */
int  csm_host_global_scan_poses(const double local_map_pose[3], const double* local_poses, int32_t n,
                                double* out_global_poses);

/* ---- pose-graph optimization: the backend's Optimize step ---- */

/* LinearSolver / SolverType of PoseGraphOptimizerLM (inc/mapping/pose_graph_optimizer_lm.hpp) */
#define CSM_PG_SOLVER_SPARSE_CHOLESKY     0   /* SimplicialLDLT: not provided (CSM_EINVAL); the direct solver
                                                 that is provided is CSM_PG_SOLVER_SCHUR_CHOLESKY */
#define CSM_PG_SOLVER_CONJUGATE_GRADIENT  1   /* Eigen ConjugateGradient<.., Lower>, Jacobi preconditioner */
#define CSM_PG_SOLVER_SCHUR_CHOLESKY      2   /* direct: the scan nodes eliminated block by block (every edge joins
                                                 a local map node to a scan node, so their 3x3 blocks are
                                                 independent), then a dense unpivoted LDL^T of the Schur
                                                 complement on the local map nodes. Not SimplicialLDLT: no
                                                 fill-reducing ordering, another elimination order, other
                                                 rounding. Trace: cg_iterations = 0, residual_norm2 = the true
                                                 |b - H delta|^2 computed after the solve. A zero or non-finite
                                                 pivot (possible only with an information matrix that is not
                                                 positive semi-definite) does not stop the call: as in the
                                                 reference, which never reads the solver's info(), the step goes
                                                 on with what the arithmetic gives. */
/* the Schur complement is stored dense ((3 n_local)^2 doubles, 1.2 GB at the cap): more local map
 * nodes than this are CSM_EINVAL under CSM_PG_SOLVER_SCHUR_CHOLESKY, on the device and on the host */
#define CSM_PG_SCHUR_MAX_LOCAL            4096

/* robust loss functions (src/mapping/robust_loss_function.cpp) */
#define CSM_PG_LOSS_SQUARED         0
#define CSM_PG_LOSS_HUBER           1
#define CSM_PG_LOSS_CAUCHY          2
#define CSM_PG_LOSS_FAIR            3
#define CSM_PG_LOSS_GEMAN_MCCLURE   4
#define CSM_PG_LOSS_WELSCH          5

/* PoseGraph::Edge as the optimizer reads it (EdgePose, inc/mapping/pose_graph.hpp):
 * start = local map node local_map_index, end = scan node scan_index */
typedef struct {
    int32_t local_map_index;     /* mLocalMapNodeIdx */
    int32_t scan_index;          /* mScanNodeIdx */
    int32_t is_loop;             /* mIsLoopConstraint: only these get the robust weight */
    int32_t reserved;
    double  relative_pose[3];    /* mRelativePose */
    double  information[9];      /* mInformationMat, row-major */
} csm_pose_graph_edge;

/* PoseGraphOptimizerLM constructor arguments (defaults: launcher_settings_default.json
 * "PoseGraphOptimizerLM": 10, 1e-4, ConjugateGradient, Huber 0.01) */
typedef struct {
    int32_t iterations_max;      /* NumOfIterationsMax, >= 1 */
    int32_t solver_type;         /* CSM_PG_SOLVER_* */
    int32_t loss_type;           /* CSM_PG_LOSS_* */
    int32_t reserved;
    double  error_tolerance;     /* ErrorTolerance */
    double  loss_scale;          /* the loss function's Scale (unused by Squared), >= 0 */
} csm_pose_graph_lm_params;

typedef struct {
    int32_t steps;               /* LM steps taken (the reference's NumOfIterations metric) */
    int32_t reserved;
    int64_t cg_iterations;       /* sum over the steps of the CG solver's iterations() */
    double  initial_error;       /* ComputeTotalError before the first step */
    double  final_error;         /* ... after the last step */
    double  final_lambda;        /* mLambda when Optimize returns (also written to *lambda) */
} csm_pose_graph_lm_info;

/* one record per LM step */
typedef struct {
    double  total_error;         /* ComputeTotalError after the step */
    double  lambda;              /* the damping factor the step's H was built with */
    double  rhs_norm2;           /* |b|^2: the CG stops once |r|^2 < max(DBL_EPSILON^2 |b|^2, DBL_MIN) */
    double  residual_norm2;      /* the CG's last recursively updated |r|^2 (0 when b = 0); SCHUR_CHOLESKY:
                                    the true |b - H delta|^2 */
    int32_t cg_iterations;       /* ConjugateGradient::iterations(): at most 2 * 3 * (n_local + n_scan);
                                    SCHUR_CHOLESKY: 0 */
    int32_t reserved;
} csm_pose_graph_lm_step;

/* PoseGraphOptimizerLM::Optimize (src/mapping/pose_graph_optimizer_lm.cpp:38-106) with the
 * ConjugateGradient solver (one launch, one workgroup, every LM step inside) or the direct
 * SchurCholesky solver (a chain of grid-wide launches per LM step, the LM state kept on the device),
 * on the device.
 * local_poses [3 * n_local] and scan_poses [3 * n_scan] are updated in place; *lambda is the
 * optimizer's mLambda, read at the start and written back at the end (it carries over between
 * calls). info and trace may be null; a trace holds iterations_max records, of which
 * info->steps are written. Runs on the ctx stream and returns when the results are on the host.
 * Deterministic; agrees with csm_host_pose_graph_lm within rounding of the reduction order
 * (DESIGN.md 4e). SparseCholesky, an index out of range, a non-finite pose, relative pose or
 * information entry, n_local < 1, iterations_max < 1, or n_local > CSM_PG_SCHUR_MAX_LOCAL under
 * SchurCholesky: CSM_EINVAL. */
int  csm_pose_graph_lm(csm_ctx* ctx, double* local_poses, int32_t n_local, double* scan_poses,
                       int32_t n_scan, const csm_pose_graph_edge* edges, int32_t n_edges,
                       const csm_pose_graph_lm_params* params, double* lambda,
                       csm_pose_graph_lm_info* info, csm_pose_graph_lm_step* trace);

/* Host only: the same, as a sequential literal restatement in double with glibc's sin / cos /
 * fmod (every sum in a fixed sequential order). The CPU reference of the above. */
int  csm_host_pose_graph_lm(double* local_poses, int32_t n_local, double* scan_poses, int32_t n_scan,
                            const csm_pose_graph_edge* edges, int32_t n_edges,
                            const csm_pose_graph_lm_params* params, double* lambda,
                            csm_pose_graph_lm_info* info, csm_pose_graph_lm_step* trace);

/* Host only: Loss(t) and Weight(t) of loss function loss_type with the given scale. */
int  csm_host_pose_graph_loss(int32_t loss_type, double scale, double squared_error, double* loss,
                              double* weight);

/* ---- pose-graph marginals: how uncertain a (local map node, scan node) pair is ----
 *
 * The covariance of the graph's estimate is the inverse of the information matrix H that one LM step
 * assembles at the given poses with lambda = 0 (the robust weight on loop edges, the 1e9 anchor on the
 * diagonal of local map node 0: every covariance is relative to the first local map, the reference's
 * gauge). The poses are inputs only. With H = [A B^T; B D] (A: local map nodes, D: scan nodes, block
 * diagonal), W_t,s = D_t^-1 B_t,s, S = A - B^T W and X = S^-1:
 *   Sigma_ss = X[s, s]
 *   Sigma_st = - sum_{s' in adj(t)} X[s, s'] W_t,s'^T                               (ascending s')
 *   Sigma_tt = D_t^-1 + sum_{s'} sum_{s''} W_t,s' X[s', s''] W_t,s''^T              (ascending s', then s'')
 *   relative = Js Sigma_ss Js^T + Js Sigma_st Je^T + Je Sigma_st^T Js^T + Je Sigma_tt Je^T
 * Js, Je: the Jacobians of InverseCompound(x_s, x_t) at the two poses, as the optimizer takes them.
 * X[r, c] is the entry in row r of column c of S^-1, solved from the LDL^T factor of S per column and
 * independently of every other column: forward y_i = e_i - sum_{k<i} L_ik y_k (k ascending), z = y / d,
 * backward x_i = z_i - sum_{k>i} L_ki x_k (k descending). Only the block columns of
 * C = {s of every pair} u adj(t of every pair) are solved. Every 3-term product runs left to right,
 * symmetric blocks are computed for i >= j and mirrored (exactly symmetric), D_t^-1 comes from the 3x3
 * LDL^T of D_t. A pair's record is therefore bit-identical whether it is requested alone or among any
 * other pairs, in any order (for a finite factor).
 *
 * CSM_EINVAL, checked on the host before any launch: the argument checks of csm_pose_graph_lm that
 * apply; n_pairs < 1; a pair index out of range (scan_index = -1 asks for the local map node alone);
 * n_local > CSM_PG_SCHUR_MAX_LOCAL; a local map node that is not connected to local map node 0 through
 * edges (S would be singular); a pair that names a scan node without edges. Scan nodes without edges
 * that no pair names take no part. An information matrix that is not positive semi-definite gives what
 * the arithmetic gives; `finite` reports it. */
typedef struct {
    int32_t local_map_index;
    int32_t scan_index;          /* -1: the local map node alone */
} csm_pose_graph_pair;

typedef struct {
    double  local_cov[9];        /* Sigma_ss, row-major */
    double  scan_cov[9];         /* Sigma_tt (zeros when scan_index = -1) */
    double  cross_cov[9];        /* Sigma_st = Cov(x_s, x_t), rows of s (zeros when -1) */
    double  relative_cov[9];     /* first-order covariance of InverseCompound(x_s, x_t) (zeros when -1) */
    int32_t finite;              /* 1 iff every entry above is finite */
    int32_t reserved;
} csm_pose_graph_marginal;

typedef struct {
    int32_t n_columns;           /* |C|: distinct local map nodes whose block columns of S^-1 were solved */
    int32_t reserved;
} csm_pose_graph_marginals_info;

/* On the device: the direct solver's kernels assemble, eliminate and factor (always the blocked path),
 * then a multi-column substitution on the factor and a thread per pair ("marginals").
 * Runs on the ctx stream and returns when the n_pairs records are on the host. Deterministic; differs
 * from csm_host_pose_graph_marginals only through the device library's sin / cos. Timers:
 * "pose_graph_marginals" (the chain), and inside it "pose_graph_marginals_factor" (the LDL^T) and
 * "pose_graph_marginals_solve" (the columns and the pairs). info may be null. */
int  csm_pose_graph_marginals(csm_ctx* ctx, const double* local_poses, int32_t n_local,
                              const double* scan_poses, int32_t n_scan, const csm_pose_graph_edge* edges,
                              int32_t n_edges, int32_t loss_type, double loss_scale,
                              const csm_pose_graph_pair* pairs, int32_t n_pairs,
                              csm_pose_graph_marginal* out, csm_pose_graph_marginals_info* info);
/* Host only: the same as a sequential restatement (glibc's sin / cos). The CPU reference of the above. */
int  csm_host_pose_graph_marginals(const double* local_poses, int32_t n_local, const double* scan_poses,
                                   int32_t n_scan, const csm_pose_graph_edge* edges, int32_t n_edges,
                                   int32_t loss_type, double loss_scale, const csm_pose_graph_pair* pairs,
                                   int32_t n_pairs, csm_pose_graph_marginal* out,
                                   csm_pose_graph_marginals_info* info);

/* Host only: the loop search window from a pair's relative_cov. out_a = min(max((2 n_sigma) *
 * sqrt(relative_cov_aa), min_range_a), max_range_a) for a = x, y, theta: the full widths range_x /
 * range_y / range_theta of csm_correlative_params / csm_bnb_params, in the local map's frame, where
 * mapLocalScanPose = InverseCompound(map pose, scan pose) lives. CSM_EINVAL: a negative or non-finite
 * diagonal entry, a negative or non-finite n_sigma, a NaN bound or min_range_a > max_range_a. */
int  csm_host_loop_search_ranges(const double relative_cov[9], double n_sigma, const double min_range[3],
                                 const double max_range[3], double out_range[3]);
/* Host only: the gate of a found loop against the graph's prediction. M = relative_cov + match_cov entry
 * by entry, read from its lower triangle; d = measured - predicted with d_theta through NormalizeAngle;
 * M = L D L^T (3x3, unpivoted, the optimizer's own), x = M^-1 d by forward, diagonal and backward
 * substitution; *chi2 = (d_0 x_0 + d_1 x_1) + d_2 x_2. A pivot that is not positive and finite: CSM_EINVAL. */
int  csm_host_loop_gate(const double relative_cov[9], const double match_cov[9], const double predicted[3],
                        const double measured[3], double* chi2);
/* Host only: out = cov^-1 through the same 3x3 LDL^T (lower triangle of cov), column j solved from the
 * unit vector e_j, entries i >= j kept and mirrored: exactly symmetric, as
 * csm_host_prior_from_robot_information and csm_host_motion_prior demand. A pivot that is not positive
 * and finite: CSM_EINVAL. */
int  csm_host_information_from_covariance(const double cov[9], double out[9]);

/* ---- loop search: the candidate pairs of a pose graph (LoopSearcherNearest::Search,
 * src/mapping/loop_searcher_nearest.cpp:59-170, per query node and for any number of query nodes) ----
 *
 * Inputs. scan_poses[n_scan][3]: global poses, the layout csm_pose_graph_lm takes (theta is not read).
 * scan_map_index[n_scan]: the local map each scan node belongs to, non-decreasing, in [0, n_maps): a local
 * map is a contiguous run of nodes. travel[n_scan]: accumulated travel distance at each node, non-decreasing
 * (csm_host_travel_distances). Nodes [0, n_ref) may be reference nodes. query_index[n_q]: scan node indices,
 * distinct, in any order; query_travel[n_q]: the travel distance a query's gate is measured from.
 *
 * A pair (query q, reference node r) is ELIGIBLE iff
 *   r < n_ref
 *   scan_map_index[r] != scan_map_index[q]
 *   !(query_travel[q] - travel[r] < travel_dist_threshold)
 *   d2 < T2, with d2 = (rx - qx) * (rx - qx) + (ry - qy) * (ry - qy)          SquaredDistance(refPose, queryPose)
 *            and  T2 = std::pow(node_dist_threshold, 2.0), computed once on the host.
 * d2 is f64 with every operation rounded on its own (no fused multiply-add), on the host and on the device:
 * the subtraction comes first and is the same operation on both, so far frames lose nothing on one side
 * that the other keeps. travel is non-decreasing and a f64 subtraction is monotone, so the third condition
 * selects a PREFIX [0, p_q) of the reference nodes: where the reference's loop leaves through `goto Done`.
 *
 * Order. The candidates of one query are ordered by (d2 ascending, then r ascending); d2 >= 0, so its bit
 * pattern orders as an unsigned 64-bit integer. The order is total: no result depends on a launch shape.
 *
 * Result per query. one_per_map = 0: the first n_per_query eligible pairs in that order. one_per_map = 1: of
 * every reference map only its first eligible pair in that order, then the first n_per_query of those (the
 * nearest reference node of each local map, the nearest maps per query node).
 *
 * Output. out[n_q * n_per_query]: query i's records in order in out[i * n_per_query ..], counts[i] of them
 * used; an unused slot is { query, -1, -1, 0, 0.0 }. info (may be NULL): pairs_evaluated = the sum of the
 * prefix lengths p_q; pairs_eligible = the sum over queries of their eligible pairs, before one_per_map and
 * before the cut to n_per_query. Both exact.
 *
 * CSM_EINVAL, on the host before any launch: a null pointer (info aside); a non-finite pose coordinate (x, y),
 * travel value, query_travel value or threshold; travel or scan_map_index decreasing; a map index outside
 * [0, n_maps); n_scan outside 1..CSM_LOOP_SEARCH_MAX_NODES; n_maps outside 1..CSM_LOOP_SEARCH_MAX_MAPS; n_ref
 * outside [0, n_scan]; a query index out of range or repeated; n_q < 1; n_per_query outside
 * 1..CSM_LOOP_SEARCH_MAX_K; one_per_map other than 0 or 1. */
#define CSM_LOOP_SEARCH_MAX_K      16
#define CSM_LOOP_SEARCH_MAX_NODES  (1 << 20)
#define CSM_LOOP_SEARCH_MAX_MAPS   (1 << 16)   /* one bit per map in the workgroup's LDS */
typedef struct {
    double  travel_dist_threshold;
    double  node_dist_threshold;
    int32_t n_per_query;            /* K: 1..CSM_LOOP_SEARCH_MAX_K */
    int32_t one_per_map;            /* 0 | 1 */
} csm_loop_search_params;

typedef struct {
    int32_t query_scan_index;
    int32_t ref_scan_index;         /* -1: an unused slot */
    int32_t ref_map_index;          /* -1: an unused slot */
    int32_t reserved;               /* 0 */
    double  dist_sq;                /* d2 */
} csm_loop_candidate;

typedef struct {
    int64_t pairs_evaluated;
    int64_t pairs_eligible;
} csm_loop_search_info;

/* Host only. out[0] = 0, out[i] = out[i-1] + std::hypot(x[i-1] - x[i], y[i-1] - y[i]): sequential, with
 * glibc's hypot, as the reference accumulates Distance(prevPose, refPose). It stays on the host: it is n
 * additions whose order is the result, and the device library's hypot is not glibc's. CSM_EINVAL: a null
 * pointer or n < 0. */
int  csm_host_travel_distances(const double* scan_poses, int32_t n, double* out);
/* Host only: the rule as a sequential restatement. The CPU reference of csm_loop_search. */
int  csm_host_loop_search(const double* scan_poses, const int32_t* scan_map_index, const double* travel,
                          int32_t n_scan, int32_t n_maps, int32_t n_ref, const int32_t* query_index,
                          const double* query_travel, int32_t n_q, const csm_loop_search_params* params,
                          csm_loop_candidate* out, int32_t* counts, csm_loop_search_info* info);
/* On the device, on the ctx stream: x, y, map index and travel uploaded as separate arrays with the query
 * table (28 bytes per node: 280 KB at 10 000 nodes), one workgroup per query (a uniform binary search for
 * the prefix; one pass over it that lists the eligible pairs in LDS; then one round per record: every lane
 * keeps the least key above the last selected one -- from the list, or from another pass over the prefix
 * when a query has more than 1 024 eligible pairs -- a wave reduction and one across the waves; with
 * one_per_map an LDS bit per map already taken), one read-back. Returns when records and counts are on the
 * host. Every byte of out, counts and info equals csm_host_loop_search's. Nothing of the graph stays
 * resident between calls. Timer: "loop_search". */
int  csm_loop_search(csm_ctx* ctx, const double* scan_poses, const int32_t* scan_map_index, const double* travel,
                     int32_t n_scan, int32_t n_maps, int32_t n_ref, const int32_t* query_index,
                     const double* query_travel, int32_t n_q, const csm_loop_search_params* params,
                     csm_loop_candidate* out, int32_t* counts, csm_loop_search_info* info);
/* Host only: the first n_total of all used records (the first counts[i] of each query's n_per_query slots),
 * ordered by (dist_sq, ref_scan_index, query_scan_index), into out[n_total]; *n_out of them. The K globally
 * nearest pairs are always among the K nearest of their own query, so with one_per_map = 0, n_per_query =
 * n_total and one query_travel for all queries this is the candidate set of LoopSearcherNearest::Search.
 * The reference cuts with std::nth_element, which leaves the choice among equal distances at the cut
 * unspecified; this function specifies it (the order above). CSM_EINVAL: a null pointer, n_q < 1,
 * n_per_query outside 1..CSM_LOOP_SEARCH_MAX_K, n_total < 0, a count outside [0, n_per_query]. */
int  csm_host_loop_candidates_nearest(const csm_loop_candidate* cands, const int32_t* counts, int32_t n_q,
                                      int32_t n_per_query, int32_t n_total, csm_loop_candidate* out,
                                      int32_t* n_out);

/* ---- loop search by appearance: polar scan descriptors matched on the device (the 2D form of ring-and-sector
 * "scan context" place recognition; the complement of csm_loop_search, which proposes by estimated pose) ----
 *
 * THE DESCRIPTOR of a scan is n_rings x n_sectors bytes, layout [ring][sector]: how many beams end in each
 * cell of a polar grid around the sensor, saturated at 255. csm_descriptor_params: n_rings in 1..32,
 * n_sectors a multiple of 4 in 4..128, range_min < range_max, both finite. Two edge tables, computed once on
 * the host in f64 with exactly these expressions (the device receives the tables and never recomputes them):
 *   ring_edge[k]   = range_min + ((range_max - range_min) * k) / n_rings,  k = 0..n_rings,   ring_edge[n_rings] = range_max
 *   sector_edge[k] = -M_PI + (2.0 * M_PI * k) / n_sectors,                 k = 0..n_sectors, sector_edge[n_sectors] = M_PI
 * A beam (a, r) is USED iff a and r are finite, ring_edge[0] <= r < ring_edge[n_rings] and sector_edge[0] <= a
 * < sector_edge[n_sectors]. Its ring is the greatest k with ring_edge[k] <= r, its sector the greatest k with
 * sector_edge[k] <= a: comparisons only, no division and no floor, so the bin is the same everywhere. A cell
 * holds min(count, 255). Counts are integers: no result depends on the order of the beams.
 * Scans are ragged: scan i is beams offsets[i] .. offsets[i + 1] of angles / ranges. out[n_scans * n_rings *
 * n_sectors]; beams_used[i] = the used beams of scan i (the others, offsets[i + 1] - offsets[i] - beams_used[i],
 * were not counted into any cell).
 * CSM_EINVAL, on the host before any launch: a null pointer; n_scans outside 1..CSM_LOOP_SEARCH_MAX_NODES;
 * offsets[0] != 0, offsets decreasing, or a scan of more than CSM_DESCRIPTOR_MAX_BEAMS beams; a parameter
 * outside the ranges above.
 *
 * THE DISTANCE of descriptors Q (query) and R (reference), with S = n_sectors and a shift s in [0, S):
 *   L1(s)         = sum over ring, sec of |Q[ring][(sec + s) mod S] - R[ring][sec]|
 *   distance      = min over s of L1(s);  shift = the smallest s that attains it
 *   ring_distance = sum over ring of |sum_sec Q[ring][sec] - sum_sec R[ring][sec]|
 * ring_distance depends on no shift and never exceeds distance (a sum of absolute values is at least the
 * absolute value of the sum). All integers: L1 <= 32 * 128 * 255 < 2^20.
 * csm_host_descriptor_shift_angle: the heading difference theta_query - theta_ref a shift implies (a feature
 * the reference sees at bearing b the query sees at b + shift * 2 pi / S), through NormalizeAngle:
 *   t = std::fmod((-(double)shift * (2.0 * M_PI)) / (double)n_sectors, 2.0 * M_PI);
 *   if (t > M_PI) t -= 2.0 * M_PI; else if (t < -M_PI) t += 2.0 * M_PI;
 * CSM_EINVAL: a null pointer, n_sectors outside the range above, shift outside [0, n_sectors).
 *
 * THE SEARCH. descriptors[n_scan][n_rings * n_sectors]; scan_map_index, travel, n_ref, query_index and
 * query_travel as csm_loop_search takes them (poses are not read). A pair (query q, reference node r) is
 * ELIGIBLE iff
 *   r < n_ref
 *   scan_map_index[r] != scan_map_index[q]
 *   !(query_travel[q] - travel[r] < travel_dist_threshold)        the prefix [0, p_q) of csm_loop_search
 *   the byte sums of both descriptors are >= min_cell_sum          (a scan that saw almost nothing matches anything)
 *   distance <= max_distance
 * Order: (distance ascending, then r ascending), total. one_per_map and the cut to n_per_query exactly as in
 * csm_loop_search. out[n_q * n_per_query], counts[n_q]; an unused slot is { query, -1, -1, 0, 0, 0 }. info (may
 * be NULL): pairs_evaluated = the sum of the prefix lengths p_q, pairs_eligible = the eligible pairs before
 * one_per_map and the cut; both exact. A pair with ring_distance > max_distance is not eligible whatever its
 * shifts say, so both implementations skip its shift search; no output can tell.
 * CSM_EINVAL, on the host before any launch: the list of csm_loop_search without the poses and the node
 * threshold (a null pointer, info aside; a non-finite travel, query_travel or travel_dist_threshold; travel or
 * scan_map_index decreasing; a map index outside [0, n_maps); n_scan, n_maps, n_ref, n_q, n_per_query,
 * one_per_map outside their ranges; a query index out of range or repeated); a descriptor parameter outside
 * its range; n_scan * n_rings * n_sectors > 2^30. */
#define CSM_DESCRIPTOR_MAX_RINGS    32
#define CSM_DESCRIPTOR_MAX_SECTORS  128
#define CSM_DESCRIPTOR_MAX_BEAMS    65536
#define CSM_APPEARANCE_REF_CHUNK    128           /* reference nodes of a query that one workgroup scores */
#define CSM_APPEARANCE_TABLE_BYTES  (64u << 20)   /* the pair table of one chunk of queries: 4 bytes per pair */
typedef struct {
    int32_t n_rings;                /* 1..CSM_DESCRIPTOR_MAX_RINGS */
    int32_t n_sectors;              /* 4..CSM_DESCRIPTOR_MAX_SECTORS, a multiple of 4 */
    double  range_min, range_max;
} csm_descriptor_params;

typedef struct {
    csm_descriptor_params descriptor;
    double   travel_dist_threshold;
    uint32_t max_distance;
    uint32_t min_cell_sum;
    int32_t  n_per_query;           /* K: 1..CSM_LOOP_SEARCH_MAX_K */
    int32_t  one_per_map;           /* 0 | 1 */
} csm_appearance_params;

typedef struct {
    int32_t  query_scan_index;
    int32_t  ref_scan_index;        /* -1: an unused slot */
    int32_t  ref_map_index;         /* -1: an unused slot */
    int32_t  shift;
    uint32_t distance;
    uint32_t ring_distance;
} csm_appearance_candidate;

/* Host only: the descriptors of n_scans ragged scans. The CPU reference of csm_scan_descriptors. */
int  csm_host_scan_descriptors(const double* angles, const double* ranges, const int32_t* offsets, int32_t n_scans,
                               const csm_descriptor_params* params, uint8_t* out, int32_t* beams_used);
/* On the device, on the ctx stream: one upload ([edge tables | offsets | angles | ranges]), one workgroup per
 * scan (the edge tables and a histogram of the cells in LDS; per beam two binary searches on the tables and one
 * integer LDS atomic), one read-back. Every byte of out and beams_used equals the host function's. Timer:
 * "scan_descriptors". */
int  csm_scan_descriptors(csm_ctx* ctx, const double* angles, const double* ranges, const int32_t* offsets,
                          int32_t n_scans, const csm_descriptor_params* params, uint8_t* out, int32_t* beams_used);
int  csm_host_descriptor_shift_angle(int32_t shift, int32_t n_sectors, double* out);
/* Host only: the rule as a sequential restatement. The CPU reference of csm_appearance_search. */
int  csm_host_appearance_search(const uint8_t* descriptors, const int32_t* scan_map_index, const double* travel,
                                int32_t n_scan, int32_t n_maps, int32_t n_ref, const int32_t* query_index,
                                const double* query_travel, int32_t n_q, const csm_appearance_params* params,
                                csm_appearance_candidate* out, int32_t* counts, csm_loop_search_info* info);
/* On the device, on the ctx stream: the descriptors, map indices, travel values and the query table uploaded
 * once (n_rings * n_sectors + 12 bytes per node: 12.9 MB at 10 000 nodes of 20 x 64; nothing stays resident
 * between calls); the ring sums of every node; then, per chunk of queries whose pair table (4 bytes per pair of
 * a query and a node below n_ref) stays within CSM_APPEARANCE_TABLE_BYTES, the scoring kernel (a workgroup per
 * query and CSM_APPEARANCE_REF_CHUNK reference nodes: the query's descriptor in LDS with its sector axis
 * doubled, in four byte phases; a wavefront per reference node, a shift per lane, v_sad_u8 on aligned dwords;
 * the minimum of L1 << 8 | s across the wave) and the selection kernel (a workgroup per query: one round per
 * record over the key distance << 32 | r, an LDS bit per map already taken); one read-back. Every byte of out,
 * counts and info equals csm_host_appearance_search's, for every launch shape. Timer: "appearance_search". */
int  csm_appearance_search(csm_ctx* ctx, const uint8_t* descriptors, const int32_t* scan_map_index,
                           const double* travel, int32_t n_scan, int32_t n_maps, int32_t n_ref,
                           const int32_t* query_index, const double* query_travel, int32_t n_q,
                           const csm_appearance_params* params, csm_appearance_candidate* out, int32_t* counts,
                           csm_loop_search_info* info);

/* ---- loop edges: pairwise consistency and the largest consistent set ----
 *
 * Do the loop edges agree with each other? Two correct closures predict the same drift; a closure onto an
 * aliased place agrees with nobody. Every pair of edges closes a cycle: its two measurements forward, the
 * current estimates backward; the cycle's error is tested against its first-order covariance.
 *
 * Inputs. local_poses[n_local][3], scan_poses[n_scan][3]: the current estimates, as csm_pose_graph_lm takes
 * them. edges[n_edges]: start = local map node s, end = scan node t, z = relative_pose = the measured
 * InverseCompound(x_s, x_t), Lambda = information; is_loop is not read. gate: the chi-square bound. The drift
 * model (all three or none): drift_var_per_metre[3], local_travel[n_local], scan_travel[n_scan] (accumulated
 * travel: csm_host_travel_distances for scan nodes; a local map takes the value of its first scan node).
 *
 * Tables, on the host (glibc; the device does no trigonometry): per edge (cos z.theta, sin z.theta) and Sigma =
 * Lambda^-1 through csm_host_information_from_covariance (exactly symmetric; a pivot that is not positive and
 * finite: CSM_EINVAL); per node that an edge names (cos theta, sin theta), once.
 *
 * The pair i < j. R(c, s) is the rotation of a table entry, J = [[0, -1], [1, 0]], p a pose's translation;
 * rotations are composed as products of table entries, never from summed angles:
 *   t_B = R_ti^T (p_tj - p_ti)      R_B = R_ti^T R_tj          scan node t_i -> t_j, estimates
 *   t_C = -R_zj^T t_zj              R_C = R_zj^T               z_j inverted
 *   t_D = R_sj^T (p_si - p_sj)                                 local map s_j -> s_i, estimates
 *   u   = t_B + R_B (t_C + R_C t_D)
 *   e_xy = t_zi + R_zi u
 *   e_th = NormalizeAngle(((z_i.th + (th_tj - th_ti)) - z_j.th) + (th_si - th_sj))
 *   J_i  = [[I, R_zi J u], [0, 1]]
 *   R_Q  = (R_zi R_B) R_C
 *   J_j  = [[-R_Q, R_Q J (t_zj - t_D)], [0, -1]]
 *   l_ij = |scan_travel[t_i] - scan_travel[t_j]| + |local_travel[s_i] - local_travel[s_j]|    (0 without a model)
 *   M    = (J_i Sigma_i J_i^T + J_j Sigma_j J_j^T) + l_ij diag(drift_var_per_metre)
 *   chi2 = e^T M^-1 e      through the optimizer's 3x3 LDL^T and substitution, as csm_host_loop_gate forms it:
 *                          (e_0 x_0 + e_1 x_1) + e_2 x_2
 * J_i, J_j: the first-order Jacobians of e in z_i and z_j. The drift term is added unrotated, which is exact
 * when its x and y entries are equal. Every operation is +, -, *, / or fmod in f64 in one fixed order (DESIGN.md
 * 4o), the same text on the host and on the device.
 *
 * Consistency. The pair (i, j), i < j, is consistent iff every pivot of M is positive and finite and chi2 <=
 * gate; a bad pivot makes it inconsistent and is counted. The relation is defined for i < j and mirrored (the
 * cycle taken from j's side is another first-order expression); the diagonal is 0. Two peaks of the same (map,
 * scan) pair are inconsistent unless they agree within their covariances; identical edges have chi2 = 0.
 *
 * Selection, integers only. Seeds: the n_seeds vertices of highest degree, ties to the lower index (n_seeds = 0
 * or >= n_edges: all). Per seed v0: K = {v0}, C = N(v0); while C is not empty take the u in C with the largest
 * |N(u) & C|, ties to the lower index, K += u, C &= N(u). The result is the largest K, ties to the seed of
 * better rank.
 *
 * Outputs. selected[n_edges] (0 | 1), degree[n_edges], info; optionally adjacency[n_edges][ceil(n_edges / 64)]
 * (bit j & 63 of word j >> 6 of row i) and chi2[n_edges][n_edges] (mirrored, zero diagonal, +inf where a pivot
 * was bad), the latter for at most CSM_LOOP_CONSISTENCY_MAX_CHI2_EDGES edges (32 MB).
 *
 * CSM_EINVAL, on the host before any launch: a null pointer (the optional ones aside); n_local or n_scan < 1;
 * n_edges outside 1..CSM_LOOP_CONSISTENCY_MAX_EDGES; an edge's node index out of range; a non-finite pose,
 * relative pose, information entry, travel value or drift variance; a negative drift variance; a negative or
 * NaN gate (+inf is allowed: every pair with good pivots is consistent); travel arrays without the variances or
 * the reverse; n_seeds < 0; chi2 asked for above its cap; an information matrix that cannot be inverted. */
#define CSM_LOOP_CONSISTENCY_MAX_EDGES       8192   /* 8 MB of adjacency */
#define CSM_LOOP_CONSISTENCY_MAX_CHI2_EDGES  2048   /* 32 MB of chi-square values */
typedef struct {
    int64_t consistent_pairs;       /* pairs i < j that are consistent */
    int64_t bad_pivots;             /* pairs i < j whose M had a pivot that is not positive and finite */
    int32_t clique_size;            /* edges selected */
    int32_t winning_seed;           /* the edge the winning search started from */
    int32_t seeds_run;
    int32_t reserved;               /* 0 */
} csm_loop_consistency_info;

/* Host only: the rule as a sequential restatement. The CPU reference of csm_loop_consistency. */
int  csm_host_loop_consistency(const double* local_poses, int32_t n_local, const double* scan_poses, int32_t n_scan,
                               const csm_pose_graph_edge* edges, int32_t n_edges, double gate,
                               const double* drift_var_per_metre, const double* local_travel,
                               const double* scan_travel, int32_t n_seeds, int32_t* selected, int32_t* degree,
                               csm_loop_consistency_info* info, uint64_t* adjacency, double* chi2);
/* On the device, on the ctx stream: one upload of the edge records (192 bytes per edge), the pair kernel (a
 * wavefront per row edge and 64 column edges, a pair per lane, the ballot is the adjacency word), degrees by
 * popcount, the seed ranking by counting, a workgroup per seed for the greedy searches, one workgroup that
 * picks the winner; one read-back. No host round trip inside the chain. Returns when the results are on the
 * host. Every byte of every output equals csm_host_loop_consistency's. Timers: "loop_consistency" (the chain),
 * and inside it "loop_consistency_pairs" and "loop_consistency_select". */
int  csm_loop_consistency(csm_ctx* ctx, const double* local_poses, int32_t n_local, const double* scan_poses,
                          int32_t n_scan, const csm_pose_graph_edge* edges, int32_t n_edges, double gate,
                          const double* drift_var_per_metre, const double* local_travel, const double* scan_travel,
                          int32_t n_seeds, int32_t* selected, int32_t* degree, csm_loop_consistency_info* info,
                          uint64_t* adjacency, double* chi2);

/* ---- measurement hooks (bench.py) ---- */
/* enable = 1: every kernel launch is bracketed by HIP events on the ctx
 * stream; enable = 2: only the dominant (fine-level) scoring kernel, to keep
 * the timed region undisturbed; 0: off. */
int  csm_enable_kernel_timing(csm_ctx* ctx, int32_t enable);
/* Drains recorded events; returns total ms and launch count since the last
 * reset for kernel "score_fine" | "score_coarse" | "bin" | "finalize" | "boxmax" |
 * "peaks_coarse" | "peaks_select" | "volume_moments" | "volume_reduce" | "prior_select" | "likelihood" |
 * "distance_columns" | "distance_rows" | "ray_project" | "ray_walk" | "pose_prep" | "pose_score" | "pose_rescore" | "pose_weights" |
 * "pose_resample" | "pose_graph" | "pose_graph_marginals" |
 * "pose_graph_marginals_factor" | "pose_graph_marginals_solve" | "loop_search" | "scan_descriptors" |
 * "appearance_search" | "loop_consistency" | "loop_consistency_pairs" | "loop_consistency_select". */
int  csm_kernel_time(csm_ctx* ctx, const char* name, double* total_ms,
                     int64_t* launches);
int  csm_reset_kernel_timing(csm_ctx* ctx);

/* Library / build identification */
const char* csm_version(void);

/* Test hook: bytes of device / pinned host memory the library holds right now, over
 * every context and group of the process. */
int  csm_debug_live_bytes(int64_t* device, int64_t* pinned);
/* Test hook: the first row and the first column of a resident map that hold a non-zero cell, as the library
 * keeps them on the host (rows, cols for a map with none): what csm_upload_grid counts, the block upload, the
 * map builder, csm_build_likelihood_map(s) and csm_build_distance_map(s) reduce on the device, and the edge-band test of every search
 * reads. out = { row, column }. CSM_ENOENT: the map is not resident. Reads host state only: no
 * synchronisation, no change to any grid. */
int  csm_debug_grid_known(csm_ctx* ctx, uint64_t map_id, int32_t out[2]);

#ifdef __cplusplus
}
#endif
#endif /* CSM_HIP_H */
